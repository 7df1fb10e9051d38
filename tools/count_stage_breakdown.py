#!/usr/bin/env python
"""Where the second counting stage spends its time, host fits against device fits.

    python tools/count_stage_breakdown.py [--clusters 45 1500] [--repeat 1]

Builds a synthetic orchard with the project's own generator (fruitnerf_amd.data.synthetic_cloud.make_export_cloud: lattice
fruits, some of them overlapping, lattice clutter), runs the GPU front-end and merge_small_clusters on it, keeps the first
N first-stage clusters and times split_large_cluster on them twice: second_stage="host" (shapes.py: KD-tree ICP and
Hausdorff, one Ward tree per hypothesis) and second_stage="device" (fit_fruits_batch: one Ward tree per cluster, one
cloud_icp and one cloud_hausdorff launch).  The pieces are timed by wrapping the functions the two paths call — the paths
themselves run unchanged; device pieces are bracketed by a device synchronisation.  Prints a Markdown table.  A tool, not
a test: bench.py does not run it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fruitnerf_amd import _kernels as K                                  # noqa: E402
from fruitnerf_amd.clustering import Clustering, PointCloud, shapes      # noqa: E402
from fruitnerf_amd.data.synthetic_cloud import make_export_cloud        # noqa: E402

H, RADIUS = 0.004, 0.03          # lattice pitch and fruit radius: ~1800 points per fruit


class Timers:
    """Accumulates the wall time spent inside wrapped functions, by label."""

    def __init__(self):
        self.seconds, self._undo = {}, []

    def wrap(self, owner, name, label, sync=False):
        fn = getattr(owner, name)

        def timed(*args, **kwargs):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kwargs)
            if sync:
                torch.cuda.synchronize()
            self.seconds[label] = self.seconds.get(label, 0.0) + time.perf_counter() - t0
            return out
        setattr(owner, name, timed)
        self._undo.append((owner, name, fn))

    def restore(self):
        for owner, name, fn in reversed(self._undo):
            setattr(owner, name, fn)
        self._undo = []


def first_stage(n_clusters: int, seed: int):
    """-> (Clustering after merge_small_clusters, the first n_clusters first-stage clusters)."""
    fruits = int(np.ceil(1.45 * n_clusters))                             # overlapping fruits share a cluster
    while True:
        X = make_export_cloud(n_fruits=fruits, seed=seed, h=H, r=RADIUS)
        cl = Clustering(template_path=None, voxel_size_down_sample=H / 4, remove_outliers_nb_points=2,
                        remove_outliers_radius=1.8 * H, min_samples=4, apple_template_size=1.0,
                        cluster_merge_distance=0.5 * RADIUS, template_radius=RADIUS)
        Xc, C, labels = cl.cluster(PointCloud(X, None, "cuda"), eps=1.8 * H, min_sampled=cl.min_samples)
        clusters, _ = cl.merge_small_clusters(Xc, C, labels)
        if len(clusters) >= n_clusters:
            cl.counter, cl.fuse_counter = n_clusters, 0               # the count is of the clusters kept
            return cl, clusters[:n_clusters], X.shape[0]
        fruits = int(np.ceil(fruits * 1.2 * n_clusters / max(len(clusters), 1)))


def run(cl, clusters, stage: str, seed: int):
    timers = Timers()
    timers.wrap(shapes, "alpha_shape", "alpha shapes")
    if stage == "host":
        timers.wrap(shapes, "ward_labels", "Ward")
        timers.wrap(shapes, "registration_icp", "ICP")
        timers.wrap(shapes, "hausdorff_distance", "Hausdorff")
    else:
        timers.wrap(shapes, "ward_tree", "Ward")
        timers.wrap(shapes, "ward_cut", "Ward")
        timers.wrap(K, "cloud_icp", "ICP", sync=True)
        timers.wrap(K, "cloud_hausdorff", "Hausdorff", sync=True)
    cl.second_stage = stage
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = cl.split_large_cluster(clusters, None, None, seed=seed)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        timers.restore()
    out = dict(timers.seconds, total=total)
    out["other"] = total - sum(timers.seconds.values())
    return count, [d["fruits"] for d in cl.cluster_decisions], out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clusters", type=int, nargs="+", default=[45, 1500])
    ap.add_argument("--repeat", type=int, default=1, help="timed runs per path (the fastest is reported)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    pieces = ["alpha shapes", "Ward", "ICP", "Hausdorff", "other", "total"]
    # first launches pay for module loading: one tiny device batch before anything is timed
    warm = Clustering(template_path=None, template_radius=RADIUS)
    warm.fit_fruits_batch([shapes.sphere_template(RADIUS, 64) + 0.001])
    rows = ["| first-stage clusters | split | path | " + " | ".join(pieces) + " | ICP + Hausdorff |",
            "|---|---|---|" + "---|" * (len(pieces) + 1)]
    notes = []
    for n in args.clusters:
        cl, clusters, n_points = first_stage(n, args.seed)
        results = {}
        for stage in ("host", "device"):
            best = None
            for _ in range(args.repeat):
                count, fruits, t = run(cl, clusters, stage, args.seed)
                if best is None or t["total"] < best[2]["total"]:
                    best = (count, fruits, t)
            results[stage] = best
        (hc, hf, ht), (dc, df, dt) = results["host"], results["device"]
        split = sum(1 for d in cl.cluster_decisions if "distances" in d)
        for stage, t in (("host", ht), ("device", dt)):
            fit = t.get("ICP", 0.0) + t.get("Hausdorff", 0.0)
            rows.append(f"| {len(clusters)} | {split} | {stage} | " + " | ".join(f"{t.get(p, 0.0):.4f}" for p in pieces) +
                        f" | {fit:.4f} |")
        hfit = ht.get("ICP", 0.0) + ht.get("Hausdorff", 0.0)
        dfit = dt.get("ICP", 0.0) + dt.get("Hausdorff", 0.0)
        rest = dt.get("alpha shapes", 0.0) + dt.get("Ward", 0.0)
        notes.append(f"N = {len(clusters)} ({n_points} cloud points, {split} split clusters): counts host {hc} / device {dc}, "
              f"{'same' if hf == df else 'DIFFERENT'} per-cluster decisions; ICP + Hausdorff host / device = "
              f"{hfit / dfit if dfit > 0 else float('nan'):.1f}x; Ward host / device = "
              f"{ht.get('Ward', 0.0) / dt['Ward'] if dt.get('Ward') else float('nan'):.1f}x; total host / device = "
              f"{ht['total'] / dt['total']:.2f}x; of the device path's total, {100 * rest / dt['total']:.0f} % is host "
              f"code (Delaunay alpha shapes {dt.get('alpha shapes', 0.0):.3f} s, Ward {dt.get('Ward', 0.0):.3f} s).")
        print(f"[count_stage_breakdown] N = {n} done", file=sys.stderr, flush=True)
    print("Seconds, wall clock.\n")
    print("\n".join(rows))
    print()
    print("\n\n".join(notes))


if __name__ == "__main__":
    main()
