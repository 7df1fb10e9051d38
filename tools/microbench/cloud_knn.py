"""kNN consumers of the depth point-cloud export on two 1 M-point clouds: the lattice export cloud of the README's
front-end figure (data/synthetic_cloud.py::make_export_cloud, defaults) and noisy sphere surfaces + clutter (the test
fixture's recipe scaled up).  Times PointCloud.remove_statistical_outlier(20, 10.0) and estimate_normals(30) on the
device (events, warm-up, repetitions: min / median / max) and the CPU library they replace — scipy's cKDTree query on
16 workers + the NumPy rule — and checks that both agree.
  python tools/microbench/cloud_knn.py [--reps 5] [--no-cpu] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fruitnerf_amd import _kernels as K                                   # noqa: E402
from fruitnerf_amd.clustering import PointCloud                           # noqa: E402
from fruitnerf_amd.data.synthetic_cloud import make_export_cloud          # noqa: E402

WORKERS = 16


def surface_cloud(scale: int = 255, seed: int = 7) -> np.ndarray:
    """tests/cloud_knn_reference.py::surface_cloud with `scale` times the points (scale 255: 994 500)."""
    rng = np.random.default_rng(seed)
    parts = []
    for c in [(-0.3, 0, 0), (0.1, 0.2, -0.1), (0.35, -0.25, 0.2)]:
        v = rng.normal(size=(1200 * scale, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        parts.append(np.array(c) + 0.05 * v + rng.normal(scale=5e-4, size=(1200 * scale, 3)))
    parts.append(rng.uniform(-0.5, 0.5, (300 * scale, 3)))
    X = np.concatenate(parts)
    X = np.concatenate([X, X[:32]])
    rng.shuffle(X)
    return X


def device_ms(fn, reps):
    fn()                                                                  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return out, {"min": min(times), "median": float(np.median(times)), "max": max(times)}


def cpu_statistical(X, nb, ratio):
    from scipy.spatial import cKDTree
    t = time.perf_counter()
    d, _ = cKDTree(X).query(X, nb, workers=WORKERS)
    avg = d.mean(axis=1)
    valid = avg > 0
    mean = avg[valid].mean()
    std = np.sqrt(((avg[valid] - mean) ** 2).sum() / (valid.sum() - 1))
    keep = valid & (avg < mean + ratio * std)
    return keep, avg, (time.perf_counter() - t) * 1e3


def cpu_normals(X, knn):
    from scipy.spatial import cKDTree
    t = time.perf_counter()
    _, idx = cKDTree(X).query(X, knn, workers=WORKERS)
    out = np.empty_like(X)
    for s in range(0, len(X), 1 << 17):                                   # chunks: [m, knn, 3] gathers
        nb = X[idx[s:s + (1 << 17)]]
        d = nb - nb.mean(axis=1, keepdims=True)
        out[s:s + (1 << 17)] = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d) / knn)[1][:, :, 0]
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cloud_knn.py times the device path: no HIP device")
    dev = torch.device("cuda:0")
    torch.set_num_threads(WORKERS)
    results = {}
    for name, X in (("export lattice cloud", make_export_cloud()), ("sphere surfaces + clutter", surface_cloud())):
        pcd = PointCloud(X, None, dev)
        r = {"points": len(X)}
        (_, kept), r["statistical_outlier_ms"] = device_ms(lambda: pcd.remove_statistical_outlier(20, 10.0), args.reps)
        _, r["estimate_normals_ms"] = device_ms(lambda: pcd.estimate_normals(30), args.reps)
        # the share of the calls that is not neighbour search: keys, sort, gather and a search that ends at the query
        _, r["knn_k1_ms"] = device_ms(lambda: K.cloud_knn(pcd.points, 1), args.reps)
        _, r["knn_k20_rows_ms"] = device_ms(lambda: K.cloud_knn(pcd.points, 20), args.reps)
        r["kept"] = int(kept.numel())
        if not args.no_cpu:
            keep_cpu, avg_cpu, r["cpu_statistical_outlier_ms"] = cpu_statistical(X, 20, 10.0)
            nrm_cpu, r["cpu_estimate_normals_ms"] = cpu_normals(X, 30)
            avg, _, _ = K.cloud_statistical_outlier(pcd.points, 20, 10.0)
            r["kept_equal_cpu"] = bool(np.array_equal(np.nonzero(keep_cpu)[0], kept.cpu().numpy()))
            r["avg_distance_max_rel_vs_cpu"] = float(np.max(np.abs(avg.cpu().numpy() - avg_cpu) / np.maximum(avg_cpu, 1e-300)))
            dots = np.abs(np.sum(pcd.normals.cpu().numpy() * nrm_cpu, axis=1))
            r["normals_share_with_dot_above_0.999999"] = float(np.mean(dots > 0.999999))
            r["speedup_statistical_outlier"] = r["cpu_statistical_outlier_ms"] / r["statistical_outlier_ms"]["median"]
            r["speedup_estimate_normals"] = r["cpu_estimate_normals_ms"] / r["estimate_normals_ms"]["median"]
        results[name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "cloud_knn_microbench.json"), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
