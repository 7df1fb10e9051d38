"""GPU: the TSDF mesh export (csrc/tsdf.hip through fruitnerf_amd/export/tsdf.py and export_tsdf_mesh) against the float64
restatement of its contract, tests/tsdf_reference.py (whose own checks run in test_tsdf_cpu.py): fusion per node, batching and
run-to-run bits, marching tetrahedra per edge key and per face, the mesh's topology, and the exporter end to end."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import tsdf_reference as tr
from tests import util

pytestmark = pytest.mark.gpu


def _tsdf(dev, lo, hi, dims, **kw):
    from fruitnerf_amd.export.tsdf import TSDF
    return TSDF.from_aabb(torch.tensor([lo, hi]), dims, dev, **kw)


def _arrays(tsdf):
    return [t.cpu().numpy() for t in (tsdf.values, tsdf.weights, tsdf.colors)]


def _compare_volume(tag, tsdf, ref, near, bound):
    """weights exact, values / colours within `bound`, on every node that is not `near` a tie or a validity edge."""
    values, weights, colors = _arrays(tsdf)
    keep = ~near
    err_v = float(np.abs(values.astype(np.float64) - ref[0])[keep].max())
    err_c = float(np.abs(colors.astype(np.float64) - ref[2])[keep].max())
    wrong_w = int((weights.astype(np.float64) != ref[1])[keep].sum())
    print(f"[{tag}] left out {int(near.sum())} of {near.size}; weights that differ {wrong_w}; max |value error| {err_v:.3g}, "
          f"max |colour error| {err_c:.3g}, bound {bound:.3g}; observed nodes {int((ref[1] > 0).sum())}")
    assert int(near.sum()) <= 0.01 * near.size
    assert wrong_w == 0
    assert err_v <= bound and err_c <= bound


# ---- fusion ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fusion():
    return tr.fusion_fixture()


def _fuse(dev, fx, kind, max_weight, masked, calls):
    tsdf = _tsdf(dev, tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, max_weight=max_weight, depth_kind=kind)
    t = {k: torch.as_tensor(v, device=dev) for k, v in fx.items()}
    depth = t["depth_ray" if kind else "depth_z"]
    for cams in calls:
        tsdf.integrate(t["c2w"][cams], t["intrinsics"][cams], depth[cams], t["rgb"][cams], t["mask"][cams] if masked else None)
    return tsdf


@pytest.mark.parametrize("max_weight", [1.0, 1e9])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_fusion_matches_the_reference(dev, fusion, masked, kind, max_weight):
    tsdf = _fuse(dev, fusion, kind, max_weight, masked, [[0, 1, 2]])
    ref, near = tr.integrate(tr.empty_volume(tr.FUSION_DIMS), tr.FUSION_LO, tr.FUSION_HI, fusion["c2w"], fusion["intrinsics"],
                             fusion["depth_ray" if kind else "depth_z"], fusion["rgb"], fusion["mask"] if masked else None,
                             depth_kind=kind, max_weight=max_weight)
    _compare_volume(f"fusion mask={masked} kind={kind} max_weight={max_weight:g}", tsdf, ref, near,
                    tr.fusion_bound(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, fusion["c2w"]))
    # the volume moved: nodes were observed from one, two and three cameras
    assert float(tsdf.weights.max()) == (1.0 if max_weight == 1.0 else 3.0) and float(tsdf.weights.min()) == 0.0


@pytest.mark.parametrize("kind,max_weight,masked", [(1, 1e9, True), (0, 1.0, False)])
def test_fusion_does_not_depend_on_batching_or_the_run(dev, fusion, kind, max_weight, masked):
    whole = _arrays(_fuse(dev, fusion, kind, max_weight, masked, [[0, 1, 2]]))
    again = _arrays(_fuse(dev, fusion, kind, max_weight, masked, [[0, 1, 2]]))
    single = _arrays(_fuse(dev, fusion, kind, max_weight, masked, [[0], [1], [2]]))
    uneven = _arrays(_fuse(dev, fusion, kind, max_weight, masked, [[0, 1], [2]]))
    for name, a, b, c, d in zip(("values", "weights", "colors"), whole, again, single, uneven):
        assert np.array_equal(a, b), f"{name}: two runs differ"
        assert np.array_equal(a, c) and np.array_equal(a, d), f"{name}: depends on how the cameras are split into calls"
    if max_weight == 1.0:                                        # the last valid camera wins: their order is part of the input
        swapped = _arrays(_fuse(dev, fusion, kind, max_weight, masked, [[2, 1, 0]]))
        assert not np.array_equal(whole[0], swapped[0])


# ---- extraction --------------------------------------------------------------------------------------------------------
def _device_mesh(dev, lo, hi, values, colors):
    tsdf = _tsdf(dev, lo, hi, values.shape)
    tsdf.values.copy_(torch.as_tensor(values))
    tsdf.colors.copy_(torch.as_tensor(colors))
    return tsdf, [t.cpu().numpy() for t in tsdf.get_mesh()]


_FIXTURES = {"field": (tr.smooth_field, tr.FIELD_LO, tr.FIELD_HI), "sphere": (tr.sphere_volume, tr.SPHERE_LO, tr.SPHERE_HI)}
_reference_meshes = {}


def _reference_mesh(name):
    if name not in _reference_meshes:
        make, lo, hi = _FIXTURES[name]
        values, colors = make()
        _reference_meshes[name] = (values, colors, tr.extract(values, colors, lo, hi))
    return _reference_meshes[name]


# A vertex coordinate in float32: the voxel size carries a relative error of one eps32 (a subtraction and a division), so
# a node coordinate lo + i * voxel_size is off by at most 3.5 ulps of the longest coordinate M (2 eps32 M from the voxel
# size at the far end of a box of extent <= 2 M, 1.5 from the product and the sum); in p_b - p_a the voxel-size error cancels
# up to one voxel's worth and leaves the 3 ulps of the two nodes' own roundings, half an ulp for the difference, t <= 1,
# and half an ulp for the last sum: 8 ulps.
_POSITION_ULPS = 8.0


@pytest.mark.parametrize("name", ["field", "sphere"])
def test_extraction_matches_the_reference(dev, name):
    _, lo, hi = _FIXTURES[name]
    values, colors, ref = _reference_mesh(name)
    if name == "field":
        assert ref["cases"] == set(range(16))
    tsdf, (vertices, faces, normals, vcolors) = _device_mesh(dev, lo, hi, values, colors)
    V, F = ref["keys"].shape[0], ref["faces"].shape[0]
    assert vertices.shape == normals.shape == vcolors.shape == (V, 3) and faces.shape == (F, 3) and V > 0 and F > 0
    assert vertices.dtype == np.float32 and faces.dtype == np.int32
    # vertices ascend by edge key: vertex k of the device is the k-th active edge of the reference
    longest = float(np.abs(tr.node_positions(lo, hi, values.shape)).max())
    err_p = float(np.abs(vertices.astype(np.float64) - ref["vertices"]).max())
    err_n = float(np.abs(normals.astype(np.float64) - ref["normals"]).max())
    print(f"[extraction {name}] V {V} F {F}; max |position error| {err_p:.3g} = {err_p / (tr.EPS32 * longest):.2f} ulps of "
          f"{longest:.3g}; max |normal error| {err_n:.3g}; colours that differ "
          f"{int((vcolors.astype(np.float64) != ref['colors']).any(1).sum())}")
    assert err_p <= _POSITION_ULPS * tr.EPS32 * longest
    assert err_n <= 1e-5
    assert np.array_equal(vcolors.astype(np.float64), ref["colors"])
    # faces as triples of edge keys: the same oriented set, and the documented order (cell, tetrahedron, triangle)
    assert int(faces.min()) >= 0 and int(faces.max()) < V
    assert tr.oriented_faces(ref["keys"][faces]) == tr.oriented_faces(ref["face_keys"])
    assert np.array_equal(faces, ref["faces"])
    # a second extraction, on a fresh workspace: identical arrays in identical order
    for a, b in zip((vertices, faces, normals, vcolors), [t.cpu().numpy() for t in tsdf.get_mesh()]):
        assert np.array_equal(a, b)


def test_device_sphere_mesh_is_a_closed_oriented_manifold(dev):
    values, colors, _ = _reference_mesh("sphere")
    _, (vertices, faces, normals, _) = _device_mesh(dev, tr.SPHERE_LO, tr.SPHERE_HI, values, colors)
    report = tr.mesh_report(vertices, faces)
    V, F = vertices.shape[0], faces.shape[0]
    delta = tr.sphere_delta()
    radius = np.linalg.norm(vertices.astype(np.float64) - np.array(tr.SPHERE_CENTER), axis=1)
    print(f"[device sphere] V {V} F {F} euler {report['euler']} volume {report['volume']:.6f} delta {delta:.6f} "
          f"max |radius - r| {np.abs(radius - tr.SPHERE_RADIUS).max():.6f}")
    assert report["closed_oriented"] and report["degenerate"] == 0 and report["used_vertices"] == V
    assert report["euler"] == 2 and F == 2 * V - 4
    assert report["volume"] > 0
    assert float(np.abs(radius - tr.SPHERE_RADIUS).max()) <= delta
    ball = lambda r: 4.0 / 3.0 * np.pi * r ** 3                           # noqa: E731
    assert ball(tr.SPHERE_RADIUS - 2 * delta) <= report["volume"] <= ball(tr.SPHERE_RADIUS + 2 * delta)
    assert float(((vertices - np.array(tr.SPHERE_CENTER)) * normals).sum(1).min()) > 0       # normals point outwards


def test_unobserved_and_empty_volumes_have_no_surface(dev):
    tsdf = _tsdf(dev, tr.FIELD_LO, tr.FIELD_HI, tr.FIELD_DIMS)
    for fill in (-1.0, 1.0, 0.0):                                # all inside; all outside; 0 counts as outside
        tsdf.values.fill_(fill)
        vertices, faces, normals, colors = tsdf.get_mesh()
        assert vertices.shape == normals.shape == colors.shape == (0, 3) and faces.shape == (0, 3)
        assert faces.dtype == torch.int32


# ---- the exporter, end to end ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    from fruitnerf_amd.cameras.cameras import Cameras
    from fruitnerf_amd.data import synthetic_apple as sa
    n_cam, HW = 3, 16
    focal = 1111.0 * HW / 800
    # density_boost 0: the rendered depth (about 0.8 from cameras on the unit sphere) ends inside the box, so the fused
    # volume has nodes on both sides of a surface (the default boost renders depth 0.1: every observed node behind it)
    oracle = util.randomize_(util.make_oracle(util.small_config(log2=4), num_images=n_cam, randomize=False), 1,
                             density_boost=0.0)
    model = util.make_hip_like(oracle, dev)
    model.eval()
    c2w = sa.make_cameras(n_cam, seed=0, device=dev).float()
    fx = torch.tensor([focal, 1.05 * focal, 0.97 * focal])
    cy = torch.tensor([8.1, 7.6, 8.3])         # not 8.0: the centre node would sit on a rounding tie of a camera that looks at it
    # the dataset's cameras are distorted; the export renders them as pinholes
    cameras = Cameras(c2w, fx, focal, 8.2, cy, width=HW, height=HW,
                      distortion_params=torch.tensor([0.2, -0.05, 0.0, 0.0, 1e-2, -1e-2]))
    pipeline = SimpleNamespace(model=model, datamanager=SimpleNamespace(train_dataset=SimpleNamespace(cameras=cameras)))
    return SimpleNamespace(model=model, cameras=cameras, pipeline=pipeline, dev=dev)


def _render(scene, factor):
    """What the exporter fuses, rendered again through a pinhole copy of the cameras: depth [n,H,W], rgb [n,H,W,3],
    semantic probabilities [n,H,W] and the intrinsics [n,4], float32 on the host."""
    from fruitnerf_amd.cameras.cameras import Cameras, generate_rays_of
    src = scene.cameras
    pin = Cameras(src.camera_to_worlds.to(scene.dev), src.fx, src.fy, src.cx, src.cy, width=src.width, height=src.height)
    pin.rescale_output_resolution(1.0 / factor)
    for k in ("fx", "fy", "cx", "cy"):
        setattr(pin, k, getattr(pin, k).to(scene.dev))
    outs = [scene.model.get_outputs_for_camera_ray_bundle(generate_rays_of(pin, i)) for i in range(len(pin))]
    stack = lambda k: torch.stack([o[k] for o in outs]).cpu().numpy()          # noqa: E731
    return {"depth": stack("depth")[..., 0], "rgb": stack("rgb"), "prob": torch.sigmoid(torch.stack(
        [o["semantics"] for o in outs]))[..., 0].cpu().numpy(),
            "intrinsics": torch.cat([pin.fx, pin.fy, pin.cx, pin.cy], 1).cpu().numpy(), "size": (pin.height, pin.width)}


@pytest.mark.parametrize("factor", [1, 2])
def test_export_tsdf_mesh_end_to_end(scene, tmp_path, factor):
    from fruitnerf_amd.export import ply
    from fruitnerf_amd.export.exporter_utils import export_tsdf_mesh
    lo, hi, dims = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (8, 8, 8)
    before = (scene.cameras.height, scene.cameras.width, scene.cameras.fx.clone())
    tsdf = export_tsdf_mesh(scene.pipeline, tmp_path / "out", downscale_factor=factor, resolution=8, batch_size=2)
    assert (scene.cameras.height, scene.cameras.width) == before[:2] and torch.equal(scene.cameras.fx, before[2])
    images = _render(scene, factor)
    assert images["size"] == (16 // factor, 16 // factor) and images["depth"].shape == (3, 16 // factor, 16 // factor)
    # the file is the mesh of the returned volume
    got = [t.cpu().numpy() for t in tsdf.get_mesh()]
    vertices, faces, normals, colors = ply.read_triangle_mesh(str(tmp_path / "out" / "tsdf_mesh.ply"))
    print(f"[export downscale={factor}] mesh: {got[0].shape[0]} vertices, {got[1].shape[0]} faces")
    assert got[0].shape[0] > 0 and got[1].shape[0] > 0
    assert np.array_equal(vertices, got[0]) and np.array_equal(faces, got[1]) and np.array_equal(normals, got[2])
    assert np.array_equal(colors, np.rint(np.clip(got[3].astype(np.float64), 0.0, 1.0) * 255.0) / 255.0)
    # the volume is the reference's, fused from the same images (distance along the ray, Nerfstudio's weight clamp)
    c2w = scene.cameras.camera_to_worlds.cpu().numpy()
    ref, near = tr.integrate(tr.empty_volume(dims), lo, hi, c2w, images["intrinsics"], images["depth"], images["rgb"],
                             depth_kind=1, max_weight=1.0)
    _compare_volume(f"export downscale={factor}", tsdf, ref, near, tr.fusion_bound(lo, hi, dims, c2w))
    assert tsdf.volume_dims == dims
    assert int((ref[0] >= 0).sum()) > 0 and int(((ref[0] < 0) & (ref[1] > 0)).sum()) > 0     # observed nodes on both sides
    if factor == 2:
        return
    # semantic_threshold: pixels below it stay out of the fusion
    middle = float(np.median(images["prob"]))
    fruit = export_tsdf_mesh(scene.pipeline, tmp_path / "fruit", downscale_factor=1, resolution=(8, 8, 8), batch_size=10,
                             semantic_threshold=middle)
    mask = images["prob"] >= np.float32(middle)
    assert 0 < int(mask.sum()) < mask.size
    ref_fruit, near = tr.integrate(tr.empty_volume(dims), lo, hi, c2w, images["intrinsics"], images["depth"], images["rgb"],
                                   mask.astype(np.uint8), depth_kind=1, max_weight=1.0)
    _compare_volume("export semantic_threshold", fruit, ref_fruit, near, tr.fusion_bound(lo, hi, dims, c2w))
    assert int((ref_fruit[1] > 0).sum()) < int((ref[1] > 0).sum())
    # above every rendered probability: nothing is fused, the mesh is empty and the file still a PLY
    nothing = export_tsdf_mesh(scene.pipeline, tmp_path / "none", downscale_factor=1, resolution=8,
                               semantic_threshold=float(images["prob"].max()) + 1e-3)
    assert float(nothing.weights.max()) == 0.0 and bool((nothing.values == -1.0).all())
    assert [tuple(t.shape) for t in nothing.get_mesh()] == [(0, 3)] * 4
    vertices, faces, normals, colors = ply.read_triangle_mesh(str(tmp_path / "none" / "tsdf_mesh.ply"))
    assert vertices.shape == faces.shape == normals.shape == colors.shape == (0, 3)
    with pytest.raises(KeyError, match="expected_depth"):
        export_tsdf_mesh(scene.pipeline, tmp_path / "bad", downscale_factor=1, resolution=8,
                         depth_output_name="expected_depth")
