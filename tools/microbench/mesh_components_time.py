"""Time of the mesh-connectivity entry points on a real export (profiles/mesh_components.md): the `fruit_nerf` shape is trained
on the synthetic apple scene (2500 steps of 4096 rays, 40 cameras of 96 x 96), export_tsdf_mesh fuses it at resolution 128 and
256, and on each mesh fnr_mesh_components, fnr_mesh_component_stats and a selection (the components of at least 24 faces) are
timed through their _kernels wrappers — allocation of the outputs and the host reads included — next to the same labels on
the host: host_components below (edge sort + scipy + relabel, the route of tests/mesh_components_reference.py) and
scipy's connected_components alone on the prebuilt graph.  Then the fruit count of export_fruit_meshes on that model.  Host clock around work that ends in a device
synchronise; medians of 7 after a warm-up.
    python tools/microbench/mesh_components_time.py"""
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)



def host_graph(faces):
    """The face graph of the contract on the host: incidences sorted by their 64-bit edge key, every face of an edge
    linked to the edge's first face.  -> CSR matrix [F, F]"""
    faces = faces.astype(np.int64)
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    face = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    real = a != b
    a, b, face = a[real], b[real], face[real]
    keys = (np.minimum(a, b) << 32) | np.maximum(a, b)
    order = np.argsort(keys, kind="stable")
    keys, face = keys[order], face[order]
    new = np.concatenate([[True], keys[1:] != keys[:-1]])
    first = face[np.flatnonzero(new)][np.cumsum(new) - 1]
    return coo_matrix((np.ones(face.size, dtype=np.int8), (face, first)), shape=(faces.shape[0],) * 2).tocsr()


def host_components(faces):
    """-> (labels numbered by first face, n): host_graph + scipy's connected_components + the relabelling"""
    F = faces.shape[0]
    n, raw = connected_components(host_graph(faces), directed=False)
    first_face = np.full(n, F, dtype=np.int64)
    np.minimum.at(first_face, raw, np.arange(F))
    rank = np.empty(n, dtype=np.int64)
    rank[np.argsort(first_face, kind="stable")] = np.arange(n)
    return rank[raw].astype(np.int32), int(n)


def trained(dev):
    from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig
    from fruitnerf_amd.data.semantics import apple_metadata
    from fruitnerf_amd.data import synthetic_apple as sa
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import FusedAdam, fused_train_iteration
    HW, focal, n_train = 96, 1111.0 * 96 / 800, 40
    scene = sa.make_scene(seed=0, device=dev)
    c2w = sa.make_cameras(n_train, seed=0, device=dev)
    data = sa.render_dataset(scene, c2w, H=HW, W=HW, fx=focal, fy=focal)
    batcher = sa.PixelBatcher(data, torch.arange(n_train, device=dev), seed=1)
    torch.manual_seed(0)
    hm = FruitModel(FruitNerfModelConfig(), apple_metadata(), num_train_data=n_train, device=dev)
    hm.train()
    opt = FusedAdam(hm, algorithm="adam")
    for step in range(2500):
        o, d, cam, batch = batcher.sample(4096)
        ld, _ = fused_train_iteration(hm, opt, RayBundle(o, d, None, cam), batch, step, want_metrics=False)
    torch.cuda.synchronize()
    print("trained:", {k: float(v) for k, v in ld.items()}, flush=True)
    hm.eval()
    return hm, c2w.float(), HW, focal, scene


def timed(fn, n=7):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out)


def main():
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.cameras.cameras import Cameras
    from fruitnerf_amd.export.exporter_utils import export_fruit_meshes, export_tsdf_mesh
    dev = torch.device("cuda:0")
    model, c2w, HW, focal, scene = trained(dev)
    cameras = Cameras(c2w, focal, focal, HW / 2, HW / 2, width=HW, height=HW)
    pipeline = SimpleNamespace(model=model, datamanager=SimpleNamespace(train_dataset=SimpleNamespace(cameras=cameras)))
    out = tempfile.mkdtemp()
    for resolution in (128, 256):
        tsdf = export_tsdf_mesh(pipeline, os.path.join(out, f"r{resolution}"), downscale_factor=1, resolution=resolution)
        mesh = tsdf.get_triangle_mesh()
        V, F = mesh.n_vertices, mesh.n_faces
        labels, n, ws = K.mesh_components(mesh.faces, V)
        sizes = torch.bincount(labels.long(), minlength=n)
        print(f"resolution {resolution}: V {V} F {F} components {n} largest {int(sizes.max())} "
              f"components under 24 faces {int((sizes < 24).sum())}", flush=True)
        t_comp = timed(lambda: K.mesh_components(mesh.faces, V))
        t_stats = timed(lambda: K.mesh_component_stats(mesh.vertices, mesh.faces, labels, n, ws))
        keep = sizes[labels.long()] >= 24
        t_sel = timed(lambda: K.mesh_select(mesh.faces, V, keep))
        faces = mesh.faces.cpu().numpy()
        t = time.perf_counter()
        ref_labels, ref_n = host_components(faces)
        t_ref = (time.perf_counter() - t) * 1e3
        graph = host_graph(faces)
        t = time.perf_counter()
        connected_components(graph, directed=False)
        t_scipy = (time.perf_counter() - t) * 1e3
        same = ref_n == n and np.array_equal(ref_labels, labels.cpu().numpy())
        print(f"  components {t_comp[0]:.3f} ms (min {t_comp[1]:.3f}); stats {t_stats[0]:.3f} ms (min {t_stats[1]:.3f}); "
              f"select {t_sel[0]:.3f} ms (min {t_sel[1]:.3f}); host reference (edge sort + scipy + relabel) {t_ref:.1f} ms, "
              f"scipy connected_components alone on the prebuilt graph {t_scipy:.1f} ms; labels equal the reference: {same}",
              flush=True)
    fruits = export_fruit_meshes(pipeline, os.path.join(out, "fruit"), downscale_factor=1, resolution=128)
    print(f"export_fruit_meshes (threshold 0.9, min 24 faces, resolution 128): {len(fruits)} fruits; the scene has "
          f"32; kept faces {fruits.mesh.n_faces} of "
          f"{fruits.full.n_faces}; closed {int(fruits.stats.closed.sum())}", flush=True)
    for r in fruits.records()[:5]:
        print("  ", r)


if __name__ == "__main__":
    main()
