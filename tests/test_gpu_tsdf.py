"""GPU: the TSDF mesh export (csrc/tsdf.hip through fruitnerf_amd/export/tsdf.py and export_tsdf_mesh) against the float64
restatement of its contract, tests/tsdf_reference.py (whose own checks run in test_tsdf_cpu.py): fusion per node, batching and
run-to-run bits, marching tetrahedra per edge key and per face, the mesh's topology, and the exporter end to end.

Beyond tr.extract's reach the reference is tr.extract_fast (held equal to extract in test_tsdf_cpu.py).  k_tsdf_mesh_scan walks
the per-block counts 1024 blocks a trip; the volumes, their blocks of 256 nodes / trips, V / F, and as measured on an MI355X
the worst position error in ulps of the longest coordinate (8 allowed) and the normals' worst |error| / (eps32 cond), for the
float32 NumPy evaluation on the CPU and for the device:

  scan 64x64x64       1024 / 1    82 059 / 161 066   0.70   0.571  0.571   one trip, exactly full: thread 1023's carry is the total
  scan 45x343x17      1025 / 2   117 089 / 226 716   0.96   0.526  0.526   a second trip of one block, which holds 251 nodes
  scan 81x81x81       2076 / 3   132 397 / 260 932   1.22   0.602  0.602   a ragged last trip and a ragged last block
  scan 128x128x128    8192 / 8   333 831 / 661 528   0.72   0.575  0.575   export_tsdf_mesh's default resolution
  checkerboard          16 / 1    14 895 /  40 500   0.31   0.673  0.673   4 owned edges per node, 12 faces per cell: face prefix 2700
  tie checkerboard      16 / 1    14 895 /  40 500   0.00   0.050  0.050   |v| = 1/2: every colour a tie, 12 181 normals exactly zero
  noise                 16 / 1    12 856 /  25 320   0.31   0.646  0.646   all 256 sign patterns of a cell
  zeros                  2 / 1       929 /   1 582   1.16   0.664  0.664   nodes of +0.0 and -0.0: t = 0 and t = 1
  field (from before)    2 / 1       857 /   1 454   1.17   0.664    -
  sphere (from before)  13 / 1     1 058 /   2 112   0.54   0.513    -

Normals: |error| <= 4 x yardstick x eps32 x cond per vertex, cond = |S| / |n| (tr.normal_condition), the yardstick being the
worst |error| / (eps32 cond) of the same formulas in float32 NumPy over the fixtures of this module: 0.673, so the kernel is
granted 2.694 and needs 0.673 (the device's figures equal the CPU's to the digits shown; the largest |normal error| is 5.6e-6,
on the checkerboard, where cond reaches 308).  Fusion: moved by (100, -200, 300) the worst value error is 1.65e-5 against a
bound of 6.9e-4 (3.7e-7 to 5.9e-7 against 6.9e-6 at the origin, special depths and weight clamps included); weights are exact.
Time on an MI355X: the module 3.1 s, of which 1.0 s is the references and the yardstick of the new volumes (computed once);
no test takes more than 0.25 s.
"""
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


def _fuse(dev, fx, kind, max_weight, masked, calls, lo=tr.FUSION_LO, hi=tr.FUSION_HI):
    tsdf = _tsdf(dev, lo, hi, tr.FUSION_DIMS, max_weight=max_weight, depth_kind=kind)
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


def _reference_fusion(fx, kind, max_weight, masked, lo=tr.FUSION_LO, hi=tr.FUSION_HI):
    return tr.integrate(tr.empty_volume(tr.FUSION_DIMS), lo, hi, fx["c2w"], fx["intrinsics"],
                        fx["depth_ray" if kind else "depth_z"], fx["rgb"], fx["mask"] if masked else None, depth_kind=kind,
                        max_weight=max_weight)


@pytest.mark.parametrize("max_weight", [1.0, 1e9])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_fusion_of_special_depths(dev, fusion, masked, kind, max_weight):
    """NaN, +inf, -1, -0.0 and 1e-30 in camera 0's depth image, on pixels that nodes project to (test_tsdf_cpu.py): +inf
    is a valid sample with s = 1, the others are none, and nothing but those nodes changes."""
    special, pixels = tr.fusion_special_depths(fusion)
    tsdf = _fuse(dev, special, kind, max_weight, masked, [[0, 1, 2]])
    ref, near = _reference_fusion(special, kind, max_weight, masked)
    _compare_volume(f"special depths mask={masked} kind={kind} max_weight={max_weight:g}", tsdf, ref, near,
                    tr.fusion_bound(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, fusion["c2w"]))
    values, weights, colors = _arrays(tsdf)
    assert bool(np.isfinite(values).all()) and bool(np.isfinite(weights).all()) and bool(np.isfinite(colors).all())
    plain, _ = _reference_fusion(fusion, kind, max_weight, masked)
    assert int((plain[1] != ref[1]).sum()) > 0                   # the special pixels changed what the reference fuses


@pytest.mark.parametrize("max_weight", [2.0, 2.5])
@pytest.mark.parametrize("kind,masked", [(0, True), (1, False)])
def test_fusion_with_a_weight_clamp_between_one_and_the_cameras(dev, fusion, kind, masked, max_weight):
    tsdf = _fuse(dev, fusion, kind, max_weight, masked, [[0, 1, 2]])
    ref, near = _reference_fusion(fusion, kind, max_weight, masked)
    _compare_volume(f"fusion mask={masked} kind={kind} max_weight={max_weight:g}", tsdf, ref, near,
                    tr.fusion_bound(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, fusion["c2w"]))
    # the clamp binds on the third camera only
    assert float(tsdf.weights.max()) == max_weight
    two = _fuse(dev, fusion, kind, max_weight, masked, [[0, 1]])
    assert float(two.weights.max()) == 2.0 and int((two.weights == 2.0).sum()) > 0
    seen, _ = _reference_fusion(fusion, kind, 1e9, masked)
    weights = tsdf.weights.cpu().numpy()
    keep = ~near
    assert int(((seen[1] == 2) & keep).sum()) > 0 and bool((weights[(seen[1] == 2) & keep] == 2.0).all())
    assert int(((seen[1] == 3) & keep).sum()) > 0 and bool((weights[(seen[1] == 3) & keep] == np.float32(max_weight)).all())
    # and a fourth observation is averaged with the clamped weight, in the reference as on the device
    tsdf.integrate(*[torch.as_tensor(fusion[k][[0]], device=dev) for k in ("c2w", "intrinsics")],
                   torch.as_tensor(fusion["depth_ray" if kind else "depth_z"][[0]], device=dev),
                   torch.as_tensor(fusion["rgb"][[0]], device=dev),
                   torch.as_tensor(fusion["mask"][[0]], device=dev) if masked else None)
    again, near4 = tr.integrate(ref, tr.FUSION_LO, tr.FUSION_HI, fusion["c2w"][[0]], fusion["intrinsics"][[0]],
                                fusion["depth_ray" if kind else "depth_z"][[0]], fusion["rgb"][[0]],
                                fusion["mask"][[0]] if masked else None, depth_kind=kind, max_weight=max_weight)
    _compare_volume(f"fourth camera max_weight={max_weight:g}", tsdf, again, near | near4,
                    tr.fusion_bound(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, fusion["c2w"]))
    assert int((again[0] != ref[0]).sum()) > 0


@pytest.mark.parametrize("kind,max_weight,masked", [(1, 1e9, True), (0, 1.0, False), (1, 1.0, False), (0, 1e9, True)])
def test_fusion_far_from_the_origin(dev, fusion, kind, max_weight, masked):
    """The scene moved by (100, -200, 300), box, nodes and cameras: the float32 bound scales with the coordinate, and the
    kernel stays inside it where it is a hundred times the bound at the origin."""
    moved, lo, hi = tr.fusion_translated(fusion, tr.FUSION_OFFSET)
    tsdf = _fuse(dev, moved, kind, max_weight, masked, [[0, 1, 2]], lo=lo, hi=hi)
    ref, near = _reference_fusion(moved, kind, max_weight, masked, lo=lo, hi=hi)
    _compare_volume(f"moved fusion mask={masked} kind={kind} max_weight={max_weight:g}", tsdf, ref, near,
                    tr.fusion_bound(lo, hi, tr.FUSION_DIMS, moved["c2w"]))
    assert float(tsdf.weights.max()) == (1.0 if max_weight == 1.0 else 3.0) and float(tsdf.weights.min()) == 0.0


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


# ---- extraction at the exporter's sizes and at the contract's edges ---------------------------------------------------
_scan = lambda dims: (lambda: tr.scan_volume(dims), tr.SCAN_LO, tr.SCAN_HI)                              # noqa: E731
_VOLUMES = {"scan 64x64x64": _scan((64, 64, 64)), "scan 45x343x17": _scan((45, 343, 17)), "scan 81x81x81": _scan((81, 81, 81)),
            "scan 128x128x128": _scan((128, 128, 128)),
            "checkerboard": (tr.checkerboard, tr.CHECKER_LO, tr.CHECKER_HI),
            "tie checkerboard": (lambda: tr.checkerboard(magnitude=0.5), tr.CHECKER_LO, tr.CHECKER_HI),
            "noise": (tr.noise_volume, tr.CHECKER_LO, tr.CHECKER_HI),
            "zeros": (tr.zeros_volume, tr.FIELD_LO, tr.FIELD_HI)}
_EXTRACT_TWICE = ("scan 45x343x17", "checkerboard")
_volumes = {}


def _volume(name):
    """(values, colors, lo, hi, extract_fast's mesh, cond per vertex) of a fixture, computed once for the module."""
    if name not in _volumes:
        make, lo, hi = _VOLUMES.get(name) or _FIXTURES[name]
        values, colors = make()
        _volumes[name] = (values, colors, lo, hi, tr.extract_fast(values, colors, lo, hi), tr.normal_condition(values, lo, hi))
    return _volumes[name]


@pytest.fixture(scope="module")
def normal_yardstick():
    """Worst |error| / (eps32 cond) of the normal's formulas evaluated in float32 NumPy, over this module's fixtures."""
    worst = 0.0
    for name in list(_FIXTURES) + list(_VOLUMES):
        values, _, lo, hi, ref, cond = _volume(name)
        worst = max(worst, tr.normal_ratio(tr.normals_float32(values, lo, hi), ref["normals"], cond))
    print(f"[normal yardstick] float32 on the CPU: worst |error| / (eps32 cond) {worst:.3f}")
    assert worst > 0.1
    return worst


def _where(node):
    block = int(node) // 256
    return f"node {int(node)}, block {block}, trip {block // tr.SCAN_BLOCKS_PER_TRIP}"


def _assert_rows_equal(tag, what, got, want, node_of_row):
    """Exact equality of two [n,3] arrays; on a mismatch, the first differing row and where its node lies in the scan."""
    assert got.shape == want.shape, f"[{tag}] {what}: shape {got.shape}, reference {want.shape}"
    bad = np.flatnonzero((got != want).any(1))
    if bad.size:
        r = int(bad[0])
        print(f"[{tag}] {what}: {bad.size} of {got.shape[0]} rows differ; the first is row {r}: device {got[r].tolist()}, "
              f"reference {want[r].tolist()} ({_where(node_of_row[r])}); the last is row {int(bad[-1])} "
              f"({_where(node_of_row[int(bad[-1])])})")
    assert bad.size == 0, f"[{tag}] {what}: {bad.size} rows differ, the first at row {int(bad[0])} ({_where(node_of_row[int(bad[0])])})"


@pytest.mark.parametrize("name", list(_VOLUMES))
def test_extraction_beyond_one_trip_of_the_block_scan_and_at_the_edges(dev, name, normal_yardstick):
    """Element by element against extract_fast: one wrong offset in one block fails.  Faces as an array (the order cell,
    tetrahedron, triangle; vertices ascending by key), colours exact, positions within _POSITION_ULPS, normals within
    4 x the float32 CPU evaluation's error relative to eps32 cond, exact zeros where the reference's normal is zero."""
    values, colors, lo, hi, ref, cond = _volume(name)
    tsdf, (vertices, faces, normals, vcolors) = _device_mesh(dev, lo, hi, values, colors)
    V, F = ref["keys"].shape[0], ref["faces"].shape[0]
    blocks = -(-values.size // 256)
    print(f"[extraction {name}] {values.size} nodes, {blocks} blocks, {-(-blocks // tr.SCAN_BLOCKS_PER_TRIP)} trips; "
          f"reference V {V} F {F}; device V {vertices.shape[0]} F {faces.shape[0]}")
    assert vertices.dtype == normals.dtype == vcolors.dtype == np.float32 and faces.dtype == np.int32
    assert (vertices.shape[0], faces.shape[0]) == (V, F)
    assert vertices.shape == normals.shape == vcolors.shape == (V, 3) and faces.shape == (F, 3)
    vertex_node, face_node = ref["keys"] // 8, ref["face_keys"].min(1) // 8      # a face's cell: its lowest edge leaves corner 0
    _assert_rows_equal(name, "faces", faces.astype(np.int64), ref["faces"], face_node)
    _assert_rows_equal(name, "colours", vcolors.astype(np.float64), ref["colors"], vertex_node)
    longest = float(np.abs(tr.node_positions(lo, hi, values.shape)).max())
    err_p = np.abs(vertices.astype(np.float64) - ref["vertices"]).max(1)
    zero = ~np.isfinite(cond)
    ratio = tr.normal_ratio(normals, ref["normals"], cond)
    err_n = np.sqrt(((normals.astype(np.float64) - ref["normals"]) ** 2).sum(1))
    worst_p, worst_n = int(err_p.argmax()), int(np.where(zero, 0.0, err_n / (tr.EPS32 * np.where(zero, 1.0, cond))).argmax())
    print(f"[extraction {name}] max |position error| {err_p.max():.3g} = {err_p.max() / (tr.EPS32 * longest):.2f} ulps of "
          f"{longest:.3g} ({_where(vertex_node[worst_p])}); normals: worst |error| / (eps32 cond) {ratio:.3f} against "
          f"{4.0 * normal_yardstick:.3f} allowed (|error| {err_n[worst_n]:.3g}, cond {cond[worst_n]:.3g}, "
          f"{_where(vertex_node[worst_n])}); largest |normal error| {err_n[~zero].max():.3g}; zero normals {int(zero.sum())}")
    assert float(err_p.max()) <= _POSITION_ULPS * tr.EPS32 * longest
    assert ratio <= 4.0 * normal_yardstick
    assert bool((normals[zero] == 0.0).all())
    assert (int(zero.sum()) > 1000 and int((~zero).sum()) > 1000) if name == "tie checkerboard" else not bool(zero.any())
    assert float(np.abs(np.linalg.norm(normals[~zero].astype(np.float64), axis=1) - 1.0).max()) <= 4.0 * tr.EPS32
    if not name.startswith("scan"):
        assert tr.oriented_faces(ref["keys"][faces]) == tr.oriented_faces(ref["face_keys"])
    if name in _EXTRACT_TWICE:                                   # a second extraction, on a fresh workspace: the same arrays
        for a, b in zip((vertices, faces, normals, vcolors), [t.cpu().numpy() for t in tsdf.get_mesh()]):
            assert np.array_equal(a, b)


_SENTINEL = -12345.0
_PAD = 64


def test_emit_writes_nothing_beyond_the_counts_it_is_given(dev):
    """fnr_tsdf_mesh_emit with n_vertices / n_faces below the totals: the rows below them are the reference's, every row at
    or past them still holds the sentinel, in all four arrays; fnr_tsdf_mesh_count reports the full totals."""
    from fruitnerf_amd import _lib as L
    lib = L.load()
    values, colors, lo, hi, ref, _ = _volume("noise")
    V, F = ref["keys"].shape[0], ref["faces"].shape[0]
    tsdf = _tsdf(dev, lo, hi, values.shape)
    tsdf.values.copy_(torch.as_tensor(values))
    tsdf.colors.copy_(torch.as_tensor(colors))
    vol = tsdf._arg
    nbytes = L.tsdf_mesh_workspace_bytes(values.size)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    L.check(lib.fnr_tsdf_mesh_count(vol.ref, L.ptr(counts), L.ptr(ws), ws.numel() * 8, L.stream_ptr(dev)), "tsdf_mesh_count")
    assert counts.tolist() == [V, F]
    whole = [t.cpu().numpy() for t in tsdf.get_mesh()]           # the wrapper's exact-size call, for the rows below the counts
    assert np.array_equal(whole[1], ref["faces"]) and np.array_equal(whole[3].astype(np.float64), ref["colors"])
    for n_vertices, n_faces in ((V, F), (V - 1, F), (V, F - 1), (V // 2, F // 3), (1, 1), (0, F), (V, 0)):
        vertices, normals, vcolors = (torch.full((V + _PAD, 3), _SENTINEL, device=dev) for _ in range(3))
        faces = torch.full((F + _PAD, 3), int(_SENTINEL), dtype=torch.int32, device=dev)
        L.check(lib.fnr_tsdf_mesh_emit(vol.ref, L.ptr(ws), ws.numel() * 8, n_vertices, n_faces, L.ptr(vertices),
                                       L.ptr(normals), L.ptr(vcolors), L.ptr(faces), L.stream_ptr(dev)), "tsdf_mesh_emit")
        torch.cuda.synchronize()
        assert counts.tolist() == [V, F]
        tag = f"n_vertices {n_vertices} of {V}, n_faces {n_faces} of {F}"
        for what, got, want, n in (("vertices", vertices, whole[0], n_vertices), ("normals", normals, whole[2], n_vertices),
                                   ("colours", vcolors, whole[3], n_vertices), ("faces", faces, whole[1], n_faces)):
            got = got.cpu().numpy()
            assert np.array_equal(got[:n], want[:n]), f"{tag}: {what} below the count differ"
            stray = np.flatnonzero((got[n:] != got.dtype.type(_SENTINEL)).any(1))
            assert stray.size == 0, f"{tag}: {what} rows at or past the count were written, the first at row {n + int(stray[0])}"
        assert np.array_equal(faces.cpu().numpy()[:n_faces], ref["faces"][:n_faces])
        assert np.array_equal(vcolors.cpu().numpy()[:n_vertices].astype(np.float64), ref["colors"][:n_vertices])
        assert float(np.abs(vertices.cpu().numpy()[:n_vertices].astype(np.float64) - ref["vertices"][:n_vertices]).max(initial=0.0)) \
            <= _POSITION_ULPS * tr.EPS32 * 1.0


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
