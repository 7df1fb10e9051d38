"""CPU: the float64 restatements the kNN GPU tests compare against are themselves checked (against scipy's k-d tree),
the fixture cloud keeps the margins that make exact comparisons fair, the PLY layout with normals round-trips, and the
new entry points reject bad arguments before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cloud_knn_reference as R


def test_reference_distances_match_scipy_kdtree():
    from scipy.spatial import cKDTree
    X, d2, _ = R.surface_knn(30)
    d, _ = cKDTree(X).query(X, 30)
    ref = np.sqrt(d2)
    rel = np.max(np.abs(ref - d) / np.maximum(d, 1e-300))
    print(f"brute force vs cKDTree: max relative distance difference {rel:.3e}")
    assert rel <= 1e-15
    # rows ascend, the first entry is the point itself or an exact duplicate of it
    assert np.all(np.diff(d2, axis=1) >= 0) and np.all(d2[:, 0] == 0)


@pytest.mark.parametrize("std_ratio", [1.0, 2.0, 10.0])
def test_fixture_keeps_a_margin_to_the_outlier_threshold(std_ratio):
    X, d2, _ = R.surface_knn(20)
    avg, keep, (mean, std, thr) = R.statistical_outlier(X, 20, std_ratio, dist2=d2)
    margin = np.min(np.abs(avg - thr)) / thr
    removed = int((~keep).sum())
    print(f"std_ratio {std_ratio}: threshold {thr:.6e}, nearest avg {margin:.3e} away (relative), {removed} removed")
    assert margin > 1e-6
    assert np.all(avg > 0)
    assert removed == {1.0: 294, 2.0: 282, 10.0: 0}[std_ratio]


def test_fixture_normals_are_well_conditioned():
    X, _, idx = R.surface_knn(30)
    gaps = R.eigen_gaps(R.covariances(X, 30, idx))
    print(f"relative eigen-gap: {np.mean(gaps < 1e-3):.4%} below 1e-3, {np.mean(gaps < 1e-2):.4%} below 1e-2")
    assert np.mean(gaps < 1e-3) <= 0.01


def test_ply_round_trip_with_and_without_normals(tmp_path):
    from fruitnerf_amd.export import ply
    rng = np.random.default_rng(0)
    pts, nrm = rng.normal(size=(37, 3)), rng.normal(size=(37, 3))
    cols = rng.integers(0, 256, (37, 3)) / 255.0
    plain, with_normals = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ply.write_point_cloud(plain, pts, cols)
    out = ply.read_point_cloud(plain)
    assert len(out) == 2 and np.array_equal(out[0], pts) and np.array_equal(out[1], cols)
    header = open(plain, "rb").read().split(b"end_header\n")[0]
    assert b"nx" not in header and len(open(plain, "rb").read()) == len(header) + len(b"end_header\n") + 37 * 27
    ply.write_point_cloud(with_normals, pts, cols, nrm)
    p, c, n = ply.read_point_cloud(with_normals)
    assert np.array_equal(p, pts) and np.array_equal(c, cols) and np.array_equal(n, nrm)
    header = open(with_normals, "rb").read().split(b"end_header\n")[0].decode("ascii")
    props = [line.split()[-1] for line in header.splitlines() if line.startswith("property")]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]           # Open3D's order
    with pytest.raises(ValueError):
        ply.write_point_cloud(with_normals, pts, cols, nrm[:5])


def test_point_cloud_methods_check_their_arguments_like_open3d():
    from fruitnerf_amd.clustering import clustering_base as cb
    pcd = cb.PointCloud(np.zeros((4, 3)), device="cpu")
    for nb, ratio in [(0, 1.0), (20, 0.0), (20, -1.0)]:
        with pytest.raises(ValueError, match="number of neighbors and standard deviation ratio must be positive"):
            pcd.remove_statistical_outlier(nb, ratio)
    with pytest.raises(ValueError):
        pcd.estimate_normals(0)
    assert pcd.normals is None
    pcd.normals = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    sel = pcd.select_by_index(torch.tensor([2, 0]))
    assert torch.equal(sel.normals, pcd.normals[[2, 0]]) and sel.colors is None


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    assert L.FNR_CLOUD_KNN_MAX == 32
    p = 64                                                     # a non-null pointer nobody reads
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1)
    big = 1 << 40
    err = lib.fnr_last_error
    assert lib.fnr_cloud_knn_workspace_bytes(1000, 20) >= lib.fnr_cloud_workspace_bytes(1000)
    # cloud_knn: null xyz, k out of range, a short / missing workspace; an empty cloud is fine
    assert lib.fnr_cloud_knn(None, 5, lo, hi, 3, p, p, p, big, None) == -1 and b"cloud_knn: null" in err()
    for k in (0, 33):
        assert lib.fnr_cloud_knn(p, 5, lo, hi, k, p, p, p, big, None) == -1 and b"cloud_knn: k" in err()
    assert lib.fnr_cloud_knn(p, 5, lo, hi, 3, p, p, p, 16, None) == -1 and b"cloud_knn: workspace" in err()
    assert lib.fnr_cloud_knn(p, 5, lo, hi, 3, p, p, None, big, None) == -1 and b"cloud_knn: workspace" in err()
    assert lib.fnr_cloud_knn(p, 5, None, hi, 3, p, p, p, big, None) == -1 and b"cloud_knn: null" in err()
    assert lib.fnr_cloud_knn(None, 0, lo, hi, 3, None, None, None, 0, None) == 0
    # statistical outlier: Open3D's argument check, then the same host checks
    for nb, ratio in [(0, 1.0), (20, 0.0)]:
        assert lib.fnr_cloud_statistical_outlier(p, 5, lo, hi, nb, ratio, p, p, p, p, big, None) == -1
        assert b"cloud_statistical_outlier: nb_neighbors and std_ratio must be positive" in err()
    assert lib.fnr_cloud_statistical_outlier(None, 5, lo, hi, 20, 1.0, p, p, p, p, big, None) == -1
    assert b"cloud_statistical_outlier: null" in err()
    assert lib.fnr_cloud_statistical_outlier(p, 5, lo, hi, 20, 1.0, p, p, p, p, 16, None) == -1
    assert b"cloud_statistical_outlier: workspace" in err()
    assert lib.fnr_cloud_estimate_normals(None, 5, lo, hi, 30, p, p, big, None) == -1
    assert b"cloud_estimate_normals: null" in err()
    assert lib.fnr_cloud_estimate_normals(p, 5, lo, hi, 40, p, p, big, None) == -1 and b"cloud_estimate_normals: k" in err()
    # depth_points: every array is required; the box comes whole or not at all
    box = (C.c_float * 3)(-1, -1, -1)
    for missing in range(4):
        args = [p, p, p, p]
        args[missing] = None
        assert lib.fnr_depth_points(*args, 8, None, None, p, p, 8, p, p, None) == -1
        assert b"depth_points: null argument" in err()
    assert lib.fnr_depth_points(p, p, p, p, 8, None, None, p, p, 8, None, p, None) == -1 and b"depth_points: null" in err()
    assert lib.fnr_depth_points(p, p, p, p, 8, box, None, p, p, 8, p, p, None) == -1 and b"box_min and box_max" in err()
    assert lib.fnr_depth_points(p, p, p, p, 0, None, None, p, p, 8, p, p, None) == 0           # an empty batch
