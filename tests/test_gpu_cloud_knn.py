"""GPU: the depth point-cloud export — exact kNN (csrc/cloud_knn.hip) against the brute force, Open3D's statistical outlier
removal and normal estimation against their NumPy restatements (tests/cloud_knn_reference.py), the rays-to-points
compaction against torch, and generate_point_cloud / export_point_cloud end to end."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cloud_knn_reference as R
from tests import util

pytestmark = pytest.mark.gpu


def _knn(dev, X, k):
    from fruitnerf_amd import _kernels as K
    d2, idx = K.cloud_knn(torch.as_tensor(np.asarray(X, dtype=np.float64).reshape(-1, 3), device=dev), k)
    torch.cuda.synchronize()
    return d2.cpu().numpy(), idx.cpu().numpy()


def _cloud(dev, X, colors=None):
    from fruitnerf_amd.clustering.clustering_base import PointCloud
    return PointCloud(X, colors, dev)


# ---- fnr_cloud_knn ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 20, 30, 32])
def test_knn_surface_cloud_equals_brute_force(dev, k):
    X, ref_d2, ref_idx = R.surface_knn(k)
    d2, idx = _knn(dev, X, k)
    assert idx.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(d2, ref_d2)


def _small_clouds():
    rng = np.random.default_rng(3)
    lattice = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    plane = np.concatenate([rng.uniform(-1, 1, (500, 2)), np.full((500, 1), 0.25)], axis=1)
    return {"lattice": (lattice, 20),                 # all ties: the index order decides
            "twelve": (rng.normal(size=(12, 3)), 20),  # n < k: padded rows
            "one": (np.array([[0.5, -2.0, 3.0]]), 5),
            "identical": (np.full((100, 3), 0.3), 20),
            "plane": (plane, 20)}


@pytest.mark.parametrize("name", ["lattice", "twelve", "one", "identical", "plane"])
def test_knn_small_clouds_equal_brute_force(dev, name):
    X, k = _small_clouds()[name]
    ref_d2, ref_idx = R.knn(X, k)
    d2, idx = _knn(dev, X, k)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(d2, ref_d2)
    if name == "twelve":
        assert np.all(idx[:, 12:] == -1) and np.all(np.isposinf(d2[:, 12:])) and np.all(idx[:, :12] >= 0)


def test_knn_empty_cloud_and_bad_k(dev):
    from fruitnerf_amd import _kernels as K
    d2, idx = K.cloud_knn(torch.empty(0, 3, dtype=torch.float64, device=dev), 20)
    assert d2.shape == (0, 20) and idx.shape == (0, 20)
    with pytest.raises(RuntimeError, match="cloud_knn"):
        K.cloud_knn(torch.zeros(5, 3, dtype=torch.float64, device=dev), 33)


# ---- remove_statistical_outlier --------------------------------------------------------------------------------------
@pytest.mark.parametrize("std_ratio", [1.0, 2.0, 10.0])
def test_statistical_outlier_matches_the_rule(dev, std_ratio):
    from fruitnerf_amd import _kernels as K
    X, ref_d2, _ = R.surface_knn(20)
    ref_avg, ref_keep, ref_stats = R.statistical_outlier(X, 20, std_ratio, dist2=ref_d2)
    colors = np.random.default_rng(5).uniform(size=X.shape)
    pcd = _cloud(dev, X, colors)
    avg, keep, stats = K.cloud_statistical_outlier(pcd.points, 20, std_ratio)
    out, kept = pcd.remove_statistical_outlier(20, std_ratio)
    avg2, keep2, stats2 = K.cloud_statistical_outlier(pcd.points, 20, std_ratio)
    torch.cuda.synchronize()
    avg_rel = np.max(np.abs(avg.cpu().numpy() - ref_avg) / ref_avg)
    stats_rel = np.max(np.abs(stats.cpu().numpy() - np.array(ref_stats)) / np.array(ref_stats))
    print(f"std_ratio {std_ratio}: avg_distance max rel {avg_rel:.3e}, stats max rel {stats_rel:.3e}, "
          f"{int((~keep).sum())} removed")
    assert avg_rel <= 1e-14
    assert stats_rel <= 1e-12
    assert np.array_equal(kept.cpu().numpy(), np.nonzero(ref_keep)[0])
    assert np.array_equal(keep.cpu().numpy(), ref_keep)
    if std_ratio == 10.0:
        assert len(out) == len(X)
    # points and colours come back in input order
    assert np.array_equal(out.points.cpu().numpy(), X[ref_keep]) and np.array_equal(out.colors.cpu().numpy(), colors[ref_keep])
    # the same call twice: the same bits
    assert torch.equal(avg, avg2) and torch.equal(keep, keep2) and torch.equal(stats, stats2)


# ---- estimate_normals ------------------------------------------------------------------------------------------------
def test_estimate_normals_match_the_eigenvectors(dev):
    X, _, ref_idx = R.surface_knn(30)
    ref, gaps = R.normals(X, 30, ref_idx)
    pcd = _cloud(dev, X)
    pcd.estimate_normals(30)
    again = _cloud(dev, X)
    again.estimate_normals()                                   # Open3D's default knn is 30
    torch.cuda.synchronize()
    assert torch.equal(pcd.normals, again.normals)             # reproducible, sign included
    got = pcd.normals.cpu().numpy()
    assert got.shape == X.shape and got.dtype == np.float64
    assert np.max(np.abs(np.linalg.norm(got, axis=1) - 1.0)) <= 1e-12
    judged = gaps >= 1e-3
    miss = 1.0 - np.abs(np.sum(got * ref, axis=1))
    print(f"normals: max 1 - |dot| {miss[judged].max():.3e} over {judged.mean():.4%} of the points")
    assert 1.0 - judged.mean() <= 0.01
    assert miss[judged].max() <= 1e-10
    # the sphere points' normals are radial
    sphere = R.surface_cloud_labels()
    on_sphere = sphere >= 0
    assert on_sphere.sum() == 3600 + 32                         # + the duplicated rows, which are sphere points
    radial = X[on_sphere] - R.SPHERE_CENTRES[sphere[on_sphere]]
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert np.all(np.abs(np.sum(got[on_sphere] * radial, axis=1)) > 0.99)


def test_estimate_normals_of_two_points(dev):
    pcd = _cloud(dev, np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]))
    pcd.estimate_normals(30)
    assert torch.equal(pcd.normals.cpu(), torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], dtype=torch.float64))


# ---- fnr_depth_points ------------------------------------------------------------------------------------------------
def test_depth_points_match_torch(dev):
    from fruitnerf_amd import _kernels as K
    g = torch.Generator().manual_seed(11)
    Rn = 1000
    o = (torch.rand(Rn, 3, generator=g) * 2 - 1).to(dev)
    d = torch.nn.functional.normalize(torch.randn(Rn, 3, generator=g), dim=-1).to(dev)
    t = (torch.rand(Rn, 1, generator=g) * 3).to(dev)
    rgb = torch.rand(Rn, 3, generator=g).to(dev)
    box = ((-2.5, -2.0, -2.5), (0.3, 2.2, 2.1))
    ref_p, ref_c = R.depth_points(o, d, t, rgb, *box)
    all_p, all_c = R.depth_points(o, d, t, rgb)
    assert 0.3 * Rn < ref_p.shape[0] < 0.7 * Rn                 # the box cuts roughly half

    def run(capacity, use_box, calls):
        points = torch.full((capacity, 3), -7.0, device=dev)
        colors = torch.full((capacity, 3), -7.0, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        for _ in range(calls):
            K.depth_points(o, d, t, rgb, box[0] if use_box else None, box[1] if use_box else None, points, colors, count)
        return points, colors, int(count.item())

    m = ref_p.shape[0]
    points, colors, cnt = run(2 * Rn, True, 1)
    assert cnt == m and torch.equal(points[:m], ref_p) and torch.equal(colors[:m], ref_c)
    assert bool((points[m:] == -7.0).all())
    points, colors, cnt = run(2 * Rn, False, 1)                # no box: every ray
    assert cnt == Rn and torch.equal(points[:Rn], all_p) and torch.equal(colors[:Rn], all_c)
    points, colors, cnt = run(2 * Rn, True, 2)                 # the running count appends
    assert cnt == 2 * m and torch.equal(points[:2 * m], torch.cat([ref_p, ref_p])) and \
        torch.equal(colors[:2 * m], torch.cat([ref_c, ref_c]))
    cap = m + m // 3                                           # too small for two calls: counted, not written
    points, colors, cnt = run(cap, True, 2)
    assert cnt == 2 * m and torch.equal(points, torch.cat([ref_p, ref_p])[:cap]) and \
        torch.equal(colors, torch.cat([ref_c, ref_c])[:cap])


# ---- generate_point_cloud / export_point_cloud -----------------------------------------------------------------------
class _Recorder:
    """pipeline.model that keeps what went in and what came out."""

    def __init__(self, model):
        self.model, self.device, self.calls = model, model.device, []

    def __call__(self, ray_bundle):
        out = self.model(ray_bundle)
        self.calls.append((ray_bundle, {k: out[k].clone() for k in ("rgb", "depth")}))
        return out


class _ReplayModel:
    def __init__(self, calls, device):
        self.outputs, self.device = iter([out for _, out in calls]), device

    def __call__(self, ray_bundle):
        return next(self.outputs)


def _replay(calls, dev):
    """A pipeline that hands out recorded ray bundles and recorded model outputs again."""
    bundles = iter([rb for rb, _ in calls])
    return SimpleNamespace(model=_ReplayModel(calls, dev),
                           datamanager=SimpleNamespace(next_train=lambda step: (next(bundles), None)))


def test_generate_point_cloud_end_to_end(dev, tmp_path):
    from fruitnerf_amd.data import synthetic_apple as sa
    from fruitnerf_amd.data.fruit_datamanager import TrainRayDataManager
    from fruitnerf_amd.export import ply
    from fruitnerf_amd.export.exporter_utils import export_point_cloud, generate_point_cloud
    n_cam, HW = 7, 24
    focal = 1111.0 * HW / 800
    data = sa.render_dataset(sa.make_scene(seed=0, device=dev), sa.make_cameras(n_cam, seed=0, device=dev), H=HW, W=HW,
                             fx=focal, fy=focal)
    model = util.make_hip_like(util.make_oracle(util.small_config(), num_images=n_cam), dev)
    model.eval()

    def datamanager():
        return TrainRayDataManager(sa.PixelBatcher(data, torch.arange(n_cam, device=dev), seed=3), 512)

    # a box whose upper x face removes about a fifth of the points (placed from one probe batch)
    with torch.no_grad():
        rb, batch = datamanager().next_train(0)
        assert rb.origins.shape == (512, 3) and batch["image"].shape == (512, 3)
        probe, _ = R.depth_points(rb.origins, rb.directions, model(rb)["depth"], model(rb)["rgb"])
    big = float(probe.abs().max()) + 1.0
    box = ((-big, -big, -big), (float(probe[:, 0].quantile(0.8)), big, big))

    rec = _Recorder(model)
    pcd = generate_point_cloud(SimpleNamespace(model=rec, datamanager=datamanager()), num_points=700,
                               remove_outliers=False, bounding_box_min=box[0], bounding_box_max=box[1])
    assert len(rec.calls) == 2                                  # the whole last batch is kept
    parts = [R.depth_points(b.origins, b.directions, out["depth"], out["rgb"], *box) for b, out in rec.calls]
    ref_p, ref_c = torch.cat([p for p, _ in parts]), torch.cat([c for _, c in parts])
    assert parts[0][0].shape[0] < 512 and 700 <= ref_p.shape[0] < 1024          # the box removes some
    assert pcd.points.dtype == torch.float64 and pcd.normals is None
    assert torch.equal(pcd.points, ref_p.double()) and torch.equal(pcd.colors, ref_c.double())

    # the filter and the normals are the two PointCloud methods on that cloud
    full = generate_point_cloud(_replay(rec.calls, dev), num_points=700, remove_outliers=True, estimate_normals=True,
                                bounding_box_min=box[0], bounding_box_max=box[1], std_ratio=1.0)
    want, kept = pcd.remove_statistical_outlier(nb_neighbors=20, std_ratio=1.0)
    want.estimate_normals()
    assert 0 < len(want) < len(pcd)
    assert torch.equal(full.points, want.points) and torch.equal(full.colors, want.colors) and \
        torch.equal(full.normals, want.normals)
    # no box: every ray of the two batches
    every = generate_point_cloud(_replay(rec.calls, dev), num_points=700, remove_outliers=False, use_bounding_box=False)
    assert len(every) == 1024
    with pytest.raises(KeyError):
        generate_point_cloud(_replay(rec.calls, dev), num_points=700, depth_output_name="expected_depth")

    # export_point_cloud: point_cloud.ply, read back unchanged up to the colour quantisation
    out = export_point_cloud(_replay(rec.calls, dev), tmp_path / "exports", num_points=700, estimate_normals=True,
                             bounding_box_min=box[0], bounding_box_max=box[1], std_ratio=1.0)
    p, c, n = ply.read_point_cloud(str(tmp_path / "exports" / "point_cloud.ply"))
    assert np.array_equal(p, want.points.cpu().numpy()) and np.array_equal(n, want.normals.cpu().numpy())
    assert np.array_equal(c, np.rint(np.clip(want.colors.cpu().numpy(), 0.0, 1.0) * 255.0) / 255.0)
    assert torch.equal(out.points, want.points)
