"""Procedural synthetic apple tree: the benchmark scene.

No dataset, checkpoint or transforms.json exists in the container, so the "synthetic apple 800x800" workload of
BASELINE.json is generated: K red fruit spheres + green foliage blobs + a brown trunk inside the unit cube,
rendered analytically (ray/sphere intersection, Lambert shading) to RGB images + binary fruit masks from M
pinhole cameras on the unit sphere looking at the origin (fx = fy = 1111, cx = cy = 400 at 800x800 — Blender's
40 degree FOV), following the conventions the reference dataparser produces after auto-scaling
(/root/reference/fruit_nerf/data/fruitnerf_dataparser.py:194-223: camera origins within the unit box, scene box
+-1) and the Nerfstudio ray convention (camera looks along -z, y up, pixel centres at +0.5).
Everything is seeded; pure torch so it runs on the HIP device (bench) or the CPU (tests, small sizes).
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

_BATCHER_SERIALS = itertools.count(1)   # PixelBatcher.serial


@dataclass
class SyntheticScene:
    centers: Tensor   # [M,3]
    radii: Tensor     # [M]
    colors: Tensor    # [M,3]
    is_fruit: Tensor  # [M] bool
    n_fruits: int


def make_scene(n_fruits: int = 32, n_foliage: int = 300, seed: int = 0, device="cpu") -> SyntheticScene:
    rng = np.random.default_rng(seed)
    fruit_c = rng.uniform(-0.35, 0.35, size=(n_fruits, 3))
    fruit_r = rng.uniform(0.03, 0.05, size=n_fruits)
    fruit_col = np.stack([rng.uniform(0.75, 0.95, n_fruits), rng.uniform(0.05, 0.2, n_fruits),
                          rng.uniform(0.05, 0.15, n_fruits)], -1)
    # foliage: blobs in a crown of radius 0.4 around (0,0,0.05)
    v = rng.normal(size=(n_foliage, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    fol_c = v * (0.4 * rng.uniform(0.2, 1.0, size=(n_foliage, 1)) ** (1 / 3)) + np.array([0, 0, 0.05])
    fol_r = rng.uniform(0.04, 0.09, size=n_foliage)
    fol_col = np.stack([rng.uniform(0.05, 0.2, n_foliage), rng.uniform(0.35, 0.7, n_foliage),
                        rng.uniform(0.05, 0.2, n_foliage)], -1)
    # trunk: chain of brown spheres below the crown
    n_trunk = 12
    trunk_c = np.stack([np.zeros(n_trunk), np.zeros(n_trunk), np.linspace(-0.75, -0.2, n_trunk)], -1)
    trunk_r = np.full(n_trunk, 0.045)
    trunk_col = np.tile(np.array([[0.35, 0.22, 0.1]]), (n_trunk, 1))
    centers = np.concatenate([fruit_c, fol_c, trunk_c])
    radii = np.concatenate([fruit_r, fol_r, trunk_r])
    colors = np.concatenate([fruit_col, fol_col, trunk_col])
    is_fruit = np.zeros(len(radii), dtype=bool)
    is_fruit[:n_fruits] = True
    f = lambda a, dt=torch.float32: torch.as_tensor(a, dtype=dt, device=device)  # noqa: E731
    return SyntheticScene(f(centers), f(radii), f(colors), torch.as_tensor(is_fruit, device=device), n_fruits)


def make_cameras(n_cameras: int = 100, seed: int = 0, device="cpu") -> Tensor:
    """camera-to-world [M,3,4]: origins on the unit sphere (upper 3/4), looking at the origin, z-up world."""
    rng = np.random.default_rng(seed + 1)
    c2w = np.zeros((n_cameras, 3, 4), dtype=np.float64)
    for i in range(n_cameras):
        phi = 2 * np.pi * (i + rng.uniform(0, 1)) / n_cameras * 7.0
        z = rng.uniform(-0.3, 0.85)
        r = np.sqrt(max(1 - z * z, 0.0))
        pos = np.array([r * np.cos(phi), r * np.sin(phi), z])
        fwd = -pos / np.linalg.norm(pos)           # viewing direction
        up = np.array([0.0, 0.0, 1.0])
        right = np.cross(fwd, up)
        right /= np.linalg.norm(right)
        true_up = np.cross(right, fwd)
        c2w[i, :, 0], c2w[i, :, 1], c2w[i, :, 2], c2w[i, :, 3] = right, true_up, -fwd, pos
    return torch.as_tensor(c2w, dtype=torch.float32, device=device)


def pixel_rays(c2w: Tensor, cam_idx: Tensor, y: Tensor, x: Tensor, fx: float, fy: float, cx: float, cy: float
               ) -> Tuple[Tensor, Tensor]:
    """Nerfstudio RayGenerator convention for pinhole cameras: pixel centre (x+0.5, y+0.5), camera -z forward."""
    dirs_cam = torch.stack([(x.float() + 0.5 - cx) / fx, -(y.float() + 0.5 - cy) / fy, -torch.ones_like(x).float()], -1)
    R = c2w[cam_idx, :, :3]
    # (a batched-GEMM einsum here costs a 58 us hipBLASLt launch per step; three fused multiply-adds do not)
    d = R[:, :, 0] * dirs_cam[:, 0:1] + R[:, :, 1] * dirs_cam[:, 1:2] + R[:, :, 2] * dirs_cam[:, 2:3]
    d = torch.nn.functional.normalize(d, dim=-1)
    o = c2w[cam_idx, :, 3]
    return o, d


def undistort_opencv(xd: Tensor, yd: Tensor, dist: Tensor) -> Tuple[Tensor, Tensor]:
    """Inverse of the OpenCV radial / tangential model (dist [..., 6] = k1, k2, k3, k4, p1, p2, broadcast against xd, yd):
    10 Newton steps from (xd, yd), a step zero where |det| <= 1e-9 — the contract of include/fruitnerf_hip.h
    (fnr_camera_table) restated in torch for data generation; not in the product path."""
    k1, k2, k3, k4, p1, p2 = dist.unbind(-1)
    x, y = xd.clone(), yd.clone()
    for _ in range(10):
        r = x * x + y * y
        d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        fx = d * x + 2.0 * p1 * x * y + p2 * (r + 2.0 * x * x) - xd
        fy = d * y + 2.0 * p2 * x * y + p1 * (r + 2.0 * y * y) - yd
        d_r = k1 + r * (2.0 * k2 + r * (3.0 * k3 + r * 4.0 * k4))
        d_x, d_y = 2.0 * x * d_r, 2.0 * y * d_r
        fx_x = d + d_x * x + 2.0 * p1 * y + 6.0 * p2 * x
        fx_y = d_y * x + 2.0 * p1 * x + 2.0 * p2 * y
        fy_x = d_x * y + 2.0 * p2 * y + 2.0 * p1 * x
        fy_y = d + d_y * y + 2.0 * p2 * x + 6.0 * p1 * y
        det = fx_x * fy_y - fx_y * fy_x
        ok = det.abs() > 1e-9
        inv = 1.0 / torch.where(ok, det, torch.ones_like(det))
        x = x - torch.where(ok, (fx * fy_y - fy * fx_y) * inv, torch.zeros_like(det))
        y = y - torch.where(ok, (fy * fx_x - fx * fy_x) * inv, torch.zeros_like(det))
    return x, y


def camera_rays(c2w_i: Tensor, y: Tensor, x: Tensor, intrinsics_i: Tensor, distortion_i: Optional[Tensor]
                ) -> Tuple[Tensor, Tensor]:
    """pixel_rays for ONE camera with its own intrinsics row (fx, fy, cx, cy) and optional OpenCV distortion row."""
    fx, fy, cx, cy = intrinsics_i.unbind(-1)
    xd, yd = (x.float() + 0.5 - cx) / fx, (y.float() + 0.5 - cy) / fy
    if distortion_i is not None:
        xd, yd = undistort_opencv(xd, yd, distortion_i)
    R = c2w_i[:, :3]
    d = R[None, :, 0] * xd[:, None] + R[None, :, 1] * (-yd)[:, None] + R[None, :, 2] * (-torch.ones_like(xd))[:, None]
    d = torch.nn.functional.normalize(d, dim=-1)
    return c2w_i[None, :, 3].expand_as(d), d


def shade_rays(scene: SyntheticScene, o: Tensor, d: Tensor, chunk: int = 1 << 18) -> Tuple[Tensor, Tensor]:
    """Analytic render: rgb [N,3] in [0,1] and fruit mask [N] (float 0/1)."""
    light = torch.nn.functional.normalize(torch.tensor([0.4, 0.3, 0.85], device=o.device), dim=0)
    rgbs, masks = [], []
    for s in range(0, o.shape[0], chunk):
        oo, dd = o[s:s + chunk], d[s:s + chunk]
        oc = oo[:, None, :] - scene.centers[None]                      # [n,M,3]
        b = (oc * dd[:, None, :]).sum(-1)
        c = (oc * oc).sum(-1) - scene.radii[None] ** 2
        disc = b * b - c
        t = -b - torch.sqrt(disc.clamp_min(0))
        t = torch.where((disc > 0) & (t > 1e-4), t, torch.full_like(t, float("inf")))
        tmin, idx = t.min(dim=1)
        hit = torch.isfinite(tmin)
        p = oo + dd * tmin.nan_to_num(posinf=0.0)[:, None]
        n = torch.nn.functional.normalize(p - scene.centers[idx], dim=-1)
        lam = 0.35 + 0.65 * (n * light).sum(-1).clamp_min(0)
        col = scene.colors[idx] * lam[:, None]
        sky = 0.85 + 0.1 * dd[:, 2:3].clamp(-1, 1)
        bg = torch.cat([sky * 0.95, sky * 0.97, sky], -1).clamp(0, 1)
        rgbs.append(torch.where(hit[:, None], col, bg))
        masks.append((hit & scene.is_fruit[idx]).float())
    return torch.cat(rgbs), torch.cat(masks)


def render_dataset(scene: SyntheticScene, c2w: Tensor, H: int = 800, W: int = 800, fx: float = 1111.0,
                   fy: float = 1111.0, intrinsics: Optional[Tensor] = None, distortion: Optional[Tensor] = None
                   ) -> Dict[str, Tensor]:
    """uint8 images [M,H,W,3] and masks [M,H,W] (the on-device 'image batch' a datamanager would hold).
    intrinsics [M,4] (fx, fy, cx, cy per image) / distortion [M,6] (k1, k2, k3, k4, p1, p2): render through per-image,
    distorted cameras (what a real capture looks like); both then come back in the dictionary."""
    dev = c2w.device
    cx, cy = W / 2.0, H / 2.0
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    imgs = torch.empty(c2w.shape[0], H, W, 3, dtype=torch.uint8, device=dev)
    msks = torch.empty(c2w.shape[0], H, W, dtype=torch.uint8, device=dev)
    per_image = intrinsics is not None or distortion is not None
    if per_image:
        if intrinsics is None:
            intrinsics = torch.tensor([fx, fy, cx, cy], dtype=torch.float32, device=dev).expand(c2w.shape[0], 4)
        intrinsics = intrinsics.to(dev, torch.float32)
        distortion = None if distortion is None else distortion.to(dev, torch.float32)
    for i in range(c2w.shape[0]):
        ci = torch.full_like(ys, i)
        if per_image:
            o, d = camera_rays(c2w[i], ys, xs, intrinsics[i], None if distortion is None else distortion[i])
        else:
            o, d = pixel_rays(c2w, ci, ys, xs, fx, fy, cx, cy)
        rgb, m = shade_rays(scene, o, d)
        imgs[i] = (rgb.view(H, W, 3) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)
        msks[i] = m.view(H, W).to(torch.uint8)
    out = {"images": imgs, "masks": msks, "H": H, "W": W, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "c2w": c2w}
    if per_image:
        out["intrinsics"], out["distortion"] = intrinsics, distortion
    return out


class PixelBatcher:
    """PixelSampler + RayGenerator of the train datamanager (data/fruit_datamanager.py:188-197) on the device:
    uniform random (image, y, x) triples -> RayBundle tensors + {"image", "fruit_mask"} batch."""

    def __init__(self, data: Dict[str, Tensor], image_ids: Tensor, seed: int, cameras=None):
        """cameras (cameras.cameras.Cameras or a nerfstudio Cameras, rows indexed like data["c2w"]): rays go through its
        per-image intrinsics and distortion (the _cams entry points) instead of the set-wide pinhole of `data`."""
        self.data = data
        self.cameras = cameras
        self._cams = None
        self.image_ids = image_ids          # dataset indices used for training (camera_indices = position here)
        self.gen = torch.Generator(device=data["images"].device)
        self.gen.manual_seed(seed)
        self._set = None
        self.serial = next(_BATCHER_SERIALS)     # never reused, unlike id()

    def program_fingerprint(self) -> tuple:
        """What a recorded step program (training.TrainingSteps) captures from this batcher by value: which batcher it is,
        the addresses of the image set (images, masks, cameras) and of the training indices, and the seed.  Host-only."""
        s = self._set
        d = self.data if s is None else {"images": s.images, "masks": s.masks, "c2w": s.c2w}
        return (self.serial, d["images"].data_ptr(), d["masks"].data_ptr(), d["c2w"].data_ptr(),
                self.image_ids.data_ptr(), self.gen.initial_seed())

    def camera_table(self):
        """K.CameraTableArg of `cameras` on the image batch's device (None without cameras): what every launch that takes
        the image set gets next to it."""
        if self.cameras is not None and self._cams is None:
            from ..cameras.cameras import camera_table_of
            self._cams = camera_table_of(self.cameras, self.data["images"].device)
        return self._cams

    def image_set(self):
        """K.ImageSetArg over the image batch (on a HIP device), built on first use and kept as `_set`."""
        if self._set is None:
            from .. import _kernels as K
            d = self.data
            self._set = K.ImageSetArg(d["images"], d["masks"], d["c2w"], d["fx"], d["fy"], d["cx"], d["cy"])
        return self._set

    def sample(self, n_rays: int, camera_optimizer=None, level0: Optional[dict] = None):
        """One fused kernel on the HIP device (fnr_sample_pixels / fnr_train_prologue); a batch on the CPU raises.
        camera_optimizer (cameras.camera_optimizers.CameraOptimizer, mode SO3xR3 or SE3): rays come from the pose-corrected
        cameras; `last_draw` keeps what training.camera_backward_and_step needs to back-propagate into the poses.
        level0 (FruitModel.level0_spec(): S, near, far, n_jitter): the whole start of the step in ONE launch
        (fnr_train_prologue: counter-based random numbers, camera adjust, pixel sampling and the proposal sampler's
        level-0 bins); `last_presample` then holds what to hand to the model as RayBundle.presampled.  With
        level0["random_background"] (background_color="random") the rays' background colours are drawn behind the prologue
        with its seed and offset (fnr_random_background) and travel as presampled["background"] [n_rays,3].  With
        level0["per_edge"] (the sampler's single_jitter off) level 0 is jittered per bin edge (fnr_train_prologue_edges) and
        `last_presample` carries per_edge, seed and offset — what the PDF levels' kernels draw from — instead of jitter rows."""
        d = self.data
        dev = d["images"].device
        if level0 is not None and dev.type == "cuda":
            from .. import _kernels as K
            pose = camera_optimizer.pose_adjustment.data if (camera_optimizer is not None and camera_optimizer.enabled) else None
            pose_mode = camera_optimizer.pose_mode if pose is not None else 0     # (without poses the mode reads nothing)
            self._offset = getattr(self, "_offset", 0) + 1
            out = K.train_prologue(self.image_set(), self.image_ids, n_rays, self.gen.initial_seed(), self._offset, pose,
                                   level0["near"], level0["far"], level0["S"], n_jitter=level0.get("n_jitter", 3),
                                   cams=self.camera_table(), pose_mode=pose_mode, per_edge=bool(level0.get("per_edge")))
            self.last_draw = {"u": out["u"], "cam": out["cam"], "c2w_adjusted": out["c2w_adjusted"]}
            self.last_presample = {"S0": out["S0"], "near": out["near"], "far": out["far"], "spacing": out["spacing"],
                                   "euclid": out["euclid"]}
            if level0.get("per_edge"):
                # one jitter per bin edge: the kernels of the PDF levels draw theirs from this seed and offset
                self.last_presample.update(per_edge=True, seed=self.gen.initial_seed(), offset=self._offset)
            else:
                self.last_presample["jitter"] = [out["jitter"][i] for i in range(out["jitter"].shape[0])]
            if level0.get("random_background"):
                self.last_presample["background"] = K.random_background(self.gen.initial_seed(), self._offset, n_rays, dev)
            return out["origins"], out["directions"], out["cam"][:, None], \
                {"image": out["image"], "fruit_mask": out["mask"][:, None]}
        u = torch.rand(n_rays, 3, device=dev, generator=self.gen)
        if dev.type == "cuda":
            from .. import _kernels as K
            iset = self.image_set()
            c2w_adj = camera_optimizer.adjusted_cameras(iset, self.image_ids) if camera_optimizer is not None else None
            o, dirs, cam, image, mask = K.sample_pixels(iset, self.image_ids, u, c2w_adj, cams=self.camera_table())
            self.last_draw = {"u": u, "cam": cam, "c2w_adjusted": c2w_adj}
            self.last_presample = None
            return o, dirs, cam[:, None], {"image": image, "fruit_mask": mask[:, None]}
        raise RuntimeError(f"PixelBatcher.sample: the image batch is on {dev}; pixel sampling + ray generation run in "
                           "libfruitnerf_hip.so on a HIP device (no CPU path; the CPU restatement is oracle/pixel_sampler.py)")
