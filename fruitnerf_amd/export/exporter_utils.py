"""sample_volume — MI355X-native mirror of /root/reference/fruit_nerf/export/exporter_utils.py:47-258.

Export loop: per batch of orthographic rays run the model in 'export' mode, threshold (density >= 70,
logit >= 3, sigmoid(logit) > 0.9), gather the three point sets, rescale.  The per-sample field queries and
the order-preserving three-stream compaction run in libfruitnerf_hip.so; Open3D object creation and PLY
writing are out of scope here — the function returns the point / colour arrays the
reference would hand to Open3D (float64, same order).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional

import torch

from .. import _kernels as K

SET_NAMES = ("semantic_colormap", "semantic", "density")
INITIAL_CAPACITY = 1 << 20   # rows per stream buffer a sample_volume call starts with (read at call time; doubled on overflow)


def _ensure_buffers(state, dev):
    cap = state["cap"]
    if state.get("buf_cap") != cap:
        state["points"] = [torch.empty(cap, 3, device=dev) for _ in range(3)]
        state["colors"] = [torch.empty(cap, 4, device=dev) for _ in range(3)]
        state["buf_cap"] = cap


def _read_counts(counts, state):
    """The three running totals on the host (pinned destination + one stream synchronize instead of a pageable
    `counts.cpu()`)."""
    dev = counts.device
    if dev.type != "cuda":                      # CPU stand-in kernels of the gloo sharding test
        return counts.tolist()
    host = state.get("counts_host")
    if host is None:
        host = state["counts_host"] = torch.empty(3, dtype=torch.int64).pin_memory()
    host.copy_(counts, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return host.tolist()


def _compact_batch(lat, ray_begin, n_rays, positions, density, rgb, logit, state):
    """One batch compacted into the front of the stream buffers; returns its three counts (one host wait, like the
    reference's per-batch .cpu(), exporter_utils.py:126-153).  Re-runs the batch with larger buffers when they
    overflow."""
    dev = density.device
    while True:
        _ensure_buffers(state, dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        K.export_compact(lat, ray_begin, n_rays, positions, density, rgb, logit, state["points"], state["colors"],
                         counts)
        c = _read_counts(counts, state)
        if max(c) <= state["cap"]:
            return c
        while state["cap"] < max(c):
            state["cap"] *= 2


def sample_volume(pipeline, num_points: int, output_dir: Optional[Path] = None, config=None,
                  transform_json: Optional[dict] = None, rank: int = 0, world_size: int = 1) -> Dict[str, dict]:
    """`pipeline` needs `.model` (FruitModel in test_mode='export' after setup_inference) and
    `.datamanager` (setup_inference done; `next_sample_volume`).  `num_points` = number of rays, as in the
    reference (exporter_utils.py:94,172).

    world_size > 1: the ray batches (x-major ray order, data/fruit_datamanager.py:105-111) are split into
    contiguous runs, one per rank; each rank compacts its batches locally and the variable-length point lists are
    all-gathered in rank order — the single-process lists, point for point, on every rank."""
    model = pipeline.model
    dm = pipeline.datamanager
    pts = {k: [] for k in SET_NAMES}
    cols = {k: [] for k in SET_NAMES}
    state = {"cap": INITIAL_CAPACITY}
    lattice = getattr(dm, "export_lattice", None)
    lat = None
    smp = getattr(model, "proposal_sampler", None)
    jittered = bool(getattr(smp, "training", False) and getattr(smp, "train_stratified", False))
    if lattice is not None and lattice["n_samples"] == getattr(model, "num_inference_samples", None) and not jittered:
        # fused lattice path: sample positions are implicit (bin centres); a jittering sampler (the reference's as-run
        # export, see components/ray_samplers.py) takes the generic path below
        lat = K.LatticeArg(lattice["xs"], lattice["ys"], lattice["zs"])
    batch = dm.orthographic_ray_generator.ray_batch_size
    n_batches = -(-num_points // batch)
    lo, hi = 0, n_batches
    if world_size > 1:
        from ..sharding import shard_range
        lo, hi = shard_range(n_batches, rank, world_size)
        dm.train_count = lo                     # batch `count` is 1-based: the next one drawn is lo + 1
    if lat is not None:
        # fused lattice path: same batches as OrthographicRayGenerator (ray_generators.py:52-58), positions implicit.
        # The compaction's counts are RUNNING totals on the device (fnr_export_compact), so the batches append to the
        # stream buffers back to back and the host waits ONCE, at the end of the pass — the point lists are the
        # per-batch lists concatenated, as before.  The pass is deterministic: if the buffers were too small it is
        # simply repeated with larger ones.
        dev = model.device
        first = dm.train_count
        while True:
            _ensure_buffers(state, dev)
            counts = torch.zeros(3, dtype=torch.int64, device=dev)
            dm.train_count = first
            for _ in range(lo, hi):
                dm.train_count += 1
                start, end = dm.orthographic_ray_generator.batch_range(dm.train_count)
                density, rgb, logit = model.export_lattice_batch(lat, lattice["direction"], start, end - start)
                K.export_compact(lat, start, end - start, None, density, rgb, logit, state["points"], state["colors"],
                                 counts)
            c = _read_counts(counts, state)
            if max(c) <= state["cap"]:
                break
            while state["cap"] < max(c):
                state["cap"] *= 2
        for s, name in enumerate(SET_NAMES):
            pts[name].append(state["points"][s][:c[s]].to("cpu", copy=True))
            cols[name].append(state["colors"][s][:c[s]].to("cpu", copy=True))
        lo = hi                                  # nothing left for the generic loop
    for _ in range(lo, hi):                      # generic path (explicit positions, e.g. the jittering sampler)
        with torch.no_grad():
            ray_bundle, _ = dm.next_sample_volume(0)
            outputs = model(ray_bundle)
        c = _compact_batch(None, 0, 0, outputs["point_location"].reshape(-1, 3),
                           outputs["density"].reshape(-1).contiguous(),
                           outputs["rgb"].reshape(-1, 3).contiguous(),
                           outputs["semantics"].reshape(-1).contiguous(), state)
        for s, name in enumerate(SET_NAMES):
            # copy=True: the stream buffers are reused by the next batch (a no-op distinction on a GPU, where the
            # transfer already copies)
            pts[name].append(state["points"][s][:c[s]].to("cpu", copy=True))
            cols[name].append(state["colors"][s][:c[s]].to("cpu", copy=True))

    if world_size > 1:
        from ..sharding import gather_chunks
        dev = model.device
        for name in SET_NAMES:
            pts[name] = [gather_chunks([t.to(dev) for t in pts[name]], world_size, torch.empty(0, 3, device=dev)).cpu()]
            cols[name] = [gather_chunks([t.to(dev) for t in cols[name]], world_size,
                                        torch.empty(0, 4, device=dev)).cpu()]

    scale = 1.0 if transform_json is None else float(transform_json["scale"])
    pcd_list = {}
    for name in SET_NAMES:
        p = torch.cat(pts[name], dim=0)
        c = torch.cat(cols[name], dim=0)
        if name != "semantic_colormap" and c.shape[0] != 0:
            c = c / c.max()  # exporter_utils.py:202-203,227-228
        # pcd.scale(1/scale) then pcd.scale(2) about the origin (exporter_utils.py:190-191,216-217,241-242)
        p = p.double() * (1.0 / scale) * 2.0
        path = None
        if output_dir is not None and config is not None:
            path = str(Path(output_dir) / config.load_dir.parts[-3] / f"{name}.ply")
        pcd_list[name] = {"points": p.numpy(), "colors": c.double().numpy()[:, :3], "path": path}
    return pcd_list


def generate_point_cloud(pipeline, num_points: int = 1_000_000, remove_outliers: bool = True,
                         estimate_normals: bool = False, rgb_output_name: str = "rgb",
                         depth_output_name: str = "depth", use_bounding_box: bool = True,
                         bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0),
                         std_ratio: float = 10.0, normal_method: str = "open3d", normal_output_name: str = "normals"):
    """Nerfstudio's generate_point_cloud (what `ns-export pointcloud` / the reference's `pointcloud` subcommand runs,
    scripts/exporter.py:49,124-129): random training rays -> a point at origin + direction * depth per ray, coloured
    with the rendered rgb -> the points strictly inside the bounding box -> Open3D's remove_statistical_outlier(20,
    std_ratio) -> optionally estimate_normals().  -> clustering.PointCloud (float64 points / colours on the device).

    `pipeline` needs `.datamanager.next_train(step)` -> (ray bundle, batch) (data/fruit_datamanager.py::
    TrainRayDataManager) and `.model(ray_bundle)` -> outputs.  Batches are drawn until at least `num_points` points are
    collected and the whole last batch is kept, as Nerfstudio does.  The points of a batch are formed, masked and
    appended to a device buffer by fnr_depth_points; the host reads the running count once per batch (Nerfstudio
    advances its progress bar there).

    normal_method (Nerfstudio's argument, as recalled): "open3d" — normals come from the cloud, if `estimate_normals`
    asks for them (unoriented); "model_output" — the model output `normal_output_name` (FruitNerfModelConfig.
    render_normals: analytic normals shaded to [0,1]) is mapped back by 2 n - 1 and travels with its point through the
    bounding-box mask (fnr_depth_points_normals) and the outlier removal into `pcd.normals` (float64, oriented);
    `estimate_normals` is then ignored.  A missing output is a KeyError, values outside [0,1] a ValueError."""
    from ..clustering.clustering_base import PointCloud
    if normal_method not in ("open3d", "model_output"):
        raise ValueError(f"normal_method {normal_method!r}: one of 'open3d', 'model_output'")
    model_normals = normal_method == "model_output"
    dev = pipeline.model.device
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    points = colors = normals = None
    have = 0
    lo = bounding_box_min if use_bounding_box else None
    hi = bounding_box_max if use_bounding_box else None
    while have < num_points:
        with torch.no_grad():
            ray_bundle, _ = pipeline.datamanager.next_train(0)
            outputs = pipeline.model(ray_bundle)
        for name in (rgb_output_name, depth_output_name):
            if name not in outputs:
                raise KeyError(f"Could not find {name} in the model outputs; choose from {list(outputs.keys())}")
        ray_normals = None
        if model_normals:
            if normal_output_name not in outputs:
                raise KeyError(f"Could not find {normal_output_name} in the model outputs; choose from "
                               f"{list(outputs.keys())}")
            ray_normals = outputs[normal_output_name].reshape(-1, 3)
            if ray_normals.numel() and not bool(((ray_normals >= 0.0) & (ray_normals <= 1.0)).all()):
                raise ValueError(f"the model output {normal_output_name} must lie in [0, 1] (shaded normals)")
            ray_normals = ray_normals * 2.0 - 1.0
        depth = outputs[depth_output_name].reshape(-1)
        need = have + depth.numel()                      # a batch appends at most one point per ray
        if points is None or need > points.shape[0]:
            cap = max(need, 2 * (0 if points is None else points.shape[0]), num_points + depth.numel())
            grown = [torch.empty(cap, 3, device=dev) for _ in range(3 if model_normals else 2)]
            if points is not None:
                grown[0][:have], grown[1][:have] = points[:have], colors[:have]
                if model_normals:
                    grown[2][:have] = normals[:have]
            points, colors = grown[:2]
            normals = grown[2] if model_normals else None
        K.depth_points(ray_bundle.origins, ray_bundle.directions, depth, outputs[rgb_output_name], lo, hi, points,
                       colors, count, normals=ray_normals, normals_out=normals)
        got = int(count.item())
        if got == have and depth.numel() == 0:
            raise RuntimeError("generate_point_cloud: the datamanager returned an empty batch")
        have = got
    pcd = PointCloud(points[:have].double(), colors[:have].double(), dev)
    if model_normals:
        pcd.normals = normals[:have].double()
    if remove_outliers:
        pcd, _ = pcd.remove_statistical_outlier(nb_neighbors=20, std_ratio=std_ratio)
    if estimate_normals and not model_normals:
        pcd.estimate_normals()
    return pcd


def export_tsdf_mesh(pipeline, output_dir, downscale_factor: int = 2, depth_output_name: str = "depth",
                     rgb_output_name: str = "rgb", resolution=128, batch_size: int = 10, use_bounding_box: bool = True,
                     bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0),
                     semantic_threshold: Optional[float] = None, min_component_faces: Optional[int] = None,
                     largest_components: Optional[int] = None, smooth_iterations: Optional[int] = None,
                     smooth_lambda: float = 0.5, smooth_mu: float = -0.53, simplify_voxel_size: Optional[float] = None):
    """Nerfstudio's ExportTSDFMesh.main / export_tsdf_mesh (`ns-export tsdf`; its fields as recalled): every camera of
    `pipeline.datamanager.train_dataset.cameras` is rendered at 1 / downscale_factor of its resolution (pinhole: the
    fusion does not model distortion, so the rays are generated without it), its `depth_output_name` / `rgb_output_name`
    images are fused into a TSDF volume of `resolution` (an int or three) nodes over the bounding box — without
    `use_bounding_box`, over `train_dataset.scene_box.aabb` — `batch_size` cameras per launch, and the marching-
    tetrahedra mesh is written to <output_dir>/tsdf_mesh.ply (ply.write_triangle_mesh).  -> the TSDF.

    semantic_threshold (this project's addition): pixels whose sigmoid(outputs["semantics"]) is below it are left out
    of the fusion, so the mesh is the fruit alone — what the counting stage looks at.  A missing output is a KeyError.

    min_component_faces / largest_components (what users of `ns-export tsdf` do next with Open3D's
    cluster_connected_triangles): the written mesh loses its connected components of fewer than min_component_faces
    faces, then keeps only its largest_components largest (export/mesh.py::TriangleMesh).  With both None the function
    makes the calls and writes the bytes it always did.  The returned TSDF is not affected.

    smooth_iterations / smooth_lambda / smooth_mu / simplify_voxel_size (what those users do before they measure
    anything: filter_smooth_taubin, simplify_vertex_clustering, compute_vertex_normals): after the component cleaning the
    written mesh is Taubin-smoothed with smooth_iterations (lambda, mu) pairs, then simplified by vertex clustering on a
    grid of simplify_voxel_size, and its normals are recomputed from its faces if either ran (_filter_mesh).  With both
    None nothing changes."""
    tsdf = _fuse_tsdf(pipeline, downscale_factor, depth_output_name, rgb_output_name, resolution, batch_size, use_bounding_box,
                      bounding_box_min, bounding_box_max, semantic_threshold)
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    if min_component_faces is None and largest_components is None and smooth_iterations is None \
            and simplify_voxel_size is None:
        tsdf.export(str(out / "tsdf_mesh.ply"))
        return tsdf
    mesh = tsdf.get_triangle_mesh()
    if min_component_faces is not None:
        mesh = mesh.remove_small_components(int(min_component_faces))
    if largest_components is not None:
        mesh = mesh.keep_largest_components(int(largest_components))
    mesh = _filter_mesh(mesh, smooth_iterations, smooth_lambda, smooth_mu, simplify_voxel_size)
    mesh.write(out / "tsdf_mesh.ply")
    return tsdf


def _filter_mesh(mesh, smooth_iterations, smooth_lambda, smooth_mu, simplify_voxel_size):
    """The filters of the mesh exporters, in their order: Taubin smoothing, vertex clustering, and vertex normals from the
    faces if either ran.  With both None the mesh itself is returned."""
    if smooth_iterations is None and simplify_voxel_size is None:
        return mesh
    if smooth_iterations is not None:
        mesh = mesh.filter_smooth_taubin(int(smooth_iterations), float(smooth_lambda), float(smooth_mu))
    if simplify_voxel_size is not None:
        mesh = mesh.simplify_vertex_clustering(float(simplify_voxel_size))
    return mesh.compute_vertex_normals()


def _fuse_tsdf(pipeline, downscale_factor, depth_output_name, rgb_output_name, resolution, batch_size, use_bounding_box,
               bounding_box_min, bounding_box_max, semantic_threshold):
    """The fusion of export_tsdf_mesh: every training camera rendered as a pinhole and fused.  -> the TSDF."""
    from ..cameras.cameras import Cameras, _column, _image_size, generate_rays_of
    from .tsdf import TSDF
    if int(downscale_factor) < 1 or int(batch_size) < 1:
        raise ValueError("export_tsdf_mesh: downscale_factor and batch_size must be at least 1")
    model = pipeline.model
    dev = model.device
    dataset = pipeline.datamanager.train_dataset
    src = dataset.cameras
    n = src.camera_to_worlds.shape[0]
    height, width = _image_size(src)
    cameras = Cameras(src.camera_to_worlds.to(dev), *[_column(getattr(src, k), n, k).to(dev) for k in ("fx", "fy", "cx", "cy")],
                      width=width, height=height, camera_type=getattr(src, "camera_type", None))
    cameras.rescale_output_resolution(1.0 / int(downscale_factor))
    if use_bounding_box:
        aabb = torch.tensor([list(bounding_box_min), list(bounding_box_max)], dtype=torch.float32)
    else:
        aabb = torch.as_tensor(dataset.scene_box.aabb, dtype=torch.float32).cpu()
    tsdf = TSDF.from_aabb(aabb, resolution, dev)
    intrinsics = torch.cat([cameras.fx, cameras.fy, cameras.cx, cameras.cy], dim=1)
    names = [depth_output_name, rgb_output_name] + ([] if semantic_threshold is None else ["semantics"])
    for begin in range(0, n, int(batch_size)):
        batch = range(begin, min(begin + int(batch_size), n))
        images = {name: [] for name in names}
        for i in batch:
            outputs = model.get_outputs_for_camera_ray_bundle(generate_rays_of(cameras, i))
            for name in names:
                if name not in outputs:
                    raise KeyError(f"Could not find {name} in the model outputs; choose from {list(outputs.keys())}")
                images[name].append(outputs[name].to(dev))
        mask = None
        if semantic_threshold is not None:
            mask = torch.sigmoid(torch.stack(images["semantics"])[..., 0]) >= float(semantic_threshold)
        tsdf.integrate(cameras.camera_to_worlds[batch.start:batch.stop], intrinsics[batch.start:batch.stop],
                       torch.stack(images[depth_output_name])[..., 0], torch.stack(images[rgb_output_name]), mask)
    return tsdf


class FruitMeshes:
    """What export_fruit_meshes returns: `mesh` (the fruit faces, small components removed), `face_component` int32 [F]
    and `stats` (export/mesh.py::ComponentStats) of that mesh, `vertex_probability` float32 [V] of the FULL mesh `full`,
    and the `tsdf`; len() is the number of fruits."""

    def __init__(self, mesh, face_component, stats, full, vertex_probability, tsdf):
        self.mesh, self.face_component, self.stats = mesh, face_component, stats
        self.full, self.vertex_probability, self.tsdf = full, vertex_probability, tsdf

    def __len__(self) -> int:
        return len(self.stats)

    def records(self):
        """One dict per fruit in component order: faces, area, volume, closed, centroid, lo, hi (host numbers)."""
        s = self.stats
        cols = {k: getattr(s, k).cpu().tolist() for k in ("n_faces", "area", "volume", "closed", "centroid", "lo", "hi")}
        return [{"faces": int(cols["n_faces"][c]), "area": cols["area"][c], "volume": cols["volume"][c],
                 "closed": bool(cols["closed"][c]), "centroid": cols["centroid"][c], "lo": cols["lo"][c],
                 "hi": cols["hi"][c]} for c in range(len(s))]


def vertex_fruit_probability(model, vertices, normals):
    """sigmoid of the field's semantic logit at every vertex [V], through the public FruitField.forward on a generic
    [V] RaySamples: origin = the vertex, direction = -normal ((0, 0, -1) where the normal is zero), starts = ends = 0.
    The model is put in eval mode for the query (the mean appearance embedding; camera index 0 is supplied for a field
    that asks for one) and restored."""
    from ..fruit_field import FieldHeadNames
    from ..rays import Frustums, RaySamples
    n = vertices.shape[0]
    if n == 0:
        return torch.empty(0, device=vertices.device)
    directions = -normals
    flat = (normals == 0).all(dim=1)
    directions[flat] = torch.tensor([0.0, 0.0, -1.0], device=vertices.device)
    zeros = torch.zeros(n, 1, device=vertices.device)
    samples = RaySamples(Frustums(vertices, directions, zeros, zeros.clone(), zeros.clone()),
                         camera_indices=torch.zeros(n, 1, dtype=torch.int32, device=vertices.device))
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            logit = model.field.forward(samples)[FieldHeadNames.SEMANTICS]
    finally:
        model.train(was_training)
    return torch.sigmoid(logit.reshape(n).float())


def export_fruit_meshes(pipeline, output_dir, semantic_threshold: float = 0.9, min_component_faces: int = 24,
                        smooth_iterations: Optional[int] = None, smooth_lambda: float = 0.5, smooth_mu: float = -0.53,
                        simplify_voxel_size: Optional[float] = None, **tsdf_arguments):
    """One surface patch per fruit, with its size.  The whole scene is fused (export_tsdf_mesh's fusion with
    `tsdf_arguments`: downscale_factor, resolution, batch_size, the bounding box, the output names — NOT its
    semantic_threshold: masking pixels leaves their nodes unobserved, unobserved nodes count as inside, and the mesh is
    then sheets between carved and never-seen space, not fruit surfaces), the mesh extracted, and every vertex labelled
    with the field's own fruit probability (vertex_fruit_probability).  The faces whose three vertices all have
    probability >= semantic_threshold (0.9: the reference's threshold, fruit_nerf.py:264) are kept, split into connected
    components, and the components of fewer than min_component_faces faces dropped.  Writes <output_dir>/fruit_mesh.ply
    and <output_dir>/fruits.json — one record per fruit in component order: faces, area, volume (signed; meaningful where
    closed), closed, centroid, lo, hi — and returns a FruitMeshes.

    smooth_iterations / smooth_lambda / smooth_mu / simplify_voxel_size: export_tsdf_mesh's filters, applied to the fruit
    mesh after the small components are gone; components and statistics are those of the FILTERED mesh (clustering can
    merge patches), so the sizes in fruits.json are sizes of the smoothed surface.  `full`, `vertex_probability` and
    `tsdf` stay those of the unfiltered scene mesh."""
    import json
    names = ("downscale_factor", "depth_output_name", "rgb_output_name", "resolution", "batch_size", "use_bounding_box",
             "bounding_box_min", "bounding_box_max")
    defaults = (2, "depth", "rgb", 128, 10, True, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    unknown = set(tsdf_arguments) - set(names)
    if unknown:
        raise TypeError(f"export_fruit_meshes: unexpected arguments {sorted(unknown)}")
    tsdf = _fuse_tsdf(pipeline, *[tsdf_arguments.get(k, d) for k, d in zip(names, defaults)], None)
    full = tsdf.get_triangle_mesh()
    probability = vertex_fruit_probability(pipeline.model, full.vertices, full.normals)
    fruit = full.select_by_vertex_mask(probability >= float(semantic_threshold))
    fruit = fruit.remove_small_components(int(min_component_faces))
    fruit = _filter_mesh(fruit, smooth_iterations, smooth_lambda, smooth_mu, simplify_voxel_size)
    face_component, _ = fruit.connected_components()
    result = FruitMeshes(fruit, face_component, fruit.component_stats(), full, probability, tsdf)
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    fruit.write(out / "fruit_mesh.ply")
    with open(out / "fruits.json", "w") as fh:
        json.dump(result.records(), fh, indent=1)
    return result


def export_point_cloud(pipeline, output_dir, **kwargs):
    """ExportPointCloud.main: generate_point_cloud(pipeline, **kwargs) written to <output_dir>/point_cloud.ply (binary
    PLY in Open3D's layout, colours quantised to uchar, normals when they were estimated).  -> the PointCloud."""
    from . import ply
    pcd = generate_point_cloud(pipeline, **kwargs)
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    ply.write_point_cloud(str(out / "point_cloud.ply"), pcd.points.cpu().numpy(), pcd.colors.cpu().numpy(),
                          None if pcd.normals is None else pcd.normals.cpu().numpy())
    return pcd
