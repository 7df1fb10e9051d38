"""Per-image intrinsics and OpenCV distortion in device ray generation (fnr_camera_table, the fnr_*_cams entry points,
fnr_camera_rays; csrc/camera_math.hpp::pixel_direction) against a float64 reference written HERE.

The contract (include/fruitnerf_hip.h): pixel (x, y) of image i -> xd = (x + 0.5 - cx_i) / fx_i, yd = (y + 0.5 - cy_i) / fy_i;
(xu, yu) solves the OpenCV forward model; the camera-frame direction is (xu, -yu, -1).  The reference solves the forward
model by Newton run to convergence in float64 and asserts its own residual.

Fixture: 6 cameras of 48 x 40 (H x W), fx in [28, 70], fy = fx * [0.95, 1.05], principal points up to 3 px off-centre,
k1 in [-0.25, 0.15], k2 in [-0.05, 0.08], |k3| <= 0.01, |k4| <= 0.002, |p1|, |p2| <= 5e-3, camera 0 undistorted;
train_ids = [0, 2, 3, 5]; u [5000, 3] (more than one CPG_ROUND of 4096 rays, no multiple of 256) with u[0] = 0.999999
and u[1] = 0."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

N_CAM, H, W, R = 6, 48, 40, 5000
TRAIN_IDS = [0, 2, 3, 5]


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def _forward_model(xu, yu, D):
    k1, k2, k3, k4, p1, p2 = [D[..., i] for i in range(6)]
    r = xu * xu + yu * yu
    d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    return (d * xu + 2 * p1 * xu * yu + p2 * (r + 2 * xu * xu), d * yu + 2 * p2 * xu * yu + p1 * (r + 2 * yu * yu))


def _undistort64(xd, yd, D, steps=60):
    """Newton on the OpenCV forward model in float64, run to convergence; returns (xu, yu, largest residual)."""
    k1, k2, k3, k4, p1, p2 = [D[..., i] for i in range(6)]
    x, y = xd.copy(), yd.copy()
    for _ in range(steps):
        r = x * x + y * y
        d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        gx, gy = _forward_model(x, y, D)
        fx, fy = gx - xd, gy - yd
        d_r = k1 + r * (2 * k2 + r * (3 * k3 + r * 4 * k4))
        d_x, d_y = 2 * x * d_r, 2 * y * d_r
        fx_x = d + d_x * x + 2 * p1 * y + 6 * p2 * x
        fx_y = d_y * x + 2 * p1 * x + 2 * p2 * y
        fy_x = d_x * y + 2 * p2 * y + 2 * p1 * x
        fy_y = d + d_y * y + 2 * p2 * x + 6 * p1 * y
        det = fx_x * fy_y - fx_y * fy_x
        x = x - (fx * fy_y - fy * fx_y) / det
        y = y - (fy * fx_x - fx * fy_x) / det
    gx, gy = _forward_model(x, y, D)
    return x, y, float(max(np.abs(gx - xd).max(), np.abs(gy - yd).max()))


def _pixels(u, n_train, Hh=H, Ww=W):
    """(slot, y, x) of the uniform numbers u, in float32 like the kernels (floor(u * n), clamped)."""
    u = torch.as_tensor(u, dtype=torch.float32)
    k = (u[:, 0] * float(n_train)).to(torch.int64).clamp_max(n_train - 1)
    y = (u[:, 1] * float(Hh)).to(torch.int64).clamp_max(Hh - 1)
    x = (u[:, 2] * float(Ww)).to(torch.int64).clamp_max(Ww - 1)
    return k.numpy(), y.numpy(), x.numpy()


def _camera_dirs64(img, y, x, Kf, Df, undistort=True):
    """Camera-frame directions [R,3] in float64 from the float32 table values; returns (dirs, residual)."""
    Kd, Dd = Kf.astype(np.float64)[img], Df.astype(np.float64)[img]
    xd = (x + 0.5 - Kd[:, 2]) / Kd[:, 0]
    yd = (y + 0.5 - Kd[:, 3]) / Kd[:, 1]
    res = 0.0
    if undistort:
        xd, yd, res = _undistort64(xd, yd, Dd)
    return np.stack([xd, -yd, -np.ones_like(xd)], -1), res


def _world_dirs64(c2w, dc):
    d = np.einsum("rab,rb->ra", c2w[:, :, :3], dc)
    return d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-12)


@pytest.fixture(scope="module")
def fx6():
    """The fixture of the module docstring, drawn from numpy.random.default_rng(0) in the order it is listed."""
    from fruitnerf_amd.data import synthetic_apple as sa
    rng = np.random.default_rng(0)
    fx = rng.uniform(28, 70, N_CAM)
    fy = fx * rng.uniform(0.95, 1.05, N_CAM)
    cx = W / 2.0 + rng.uniform(-3, 3, N_CAM)
    cy = H / 2.0 + rng.uniform(-3, 3, N_CAM)
    k1 = rng.uniform(-0.25, 0.15, N_CAM)
    k2 = rng.uniform(-0.05, 0.08, N_CAM)
    k3 = rng.uniform(-0.01, 0.01, N_CAM)
    k4 = rng.uniform(-0.002, 0.002, N_CAM)
    p1 = rng.uniform(-5e-3, 5e-3, N_CAM)
    p2 = rng.uniform(-5e-3, 5e-3, N_CAM)
    Kf = np.stack([fx, fy, cx, cy], -1).astype(np.float32)
    Df = np.stack([k1, k2, k3, k4, p1, p2], -1).astype(np.float32)
    Df[0] = 0.0
    u = rng.uniform(0, 1, (R, 3)).astype(np.float32)
    u[0], u[1] = 0.999999, 0.0
    images = rng.integers(0, 256, (N_CAM, H, W, 3)).astype(np.uint8)
    masks = rng.integers(0, 2, (N_CAM, H, W)).astype(np.uint8)
    c2w = sa.make_cameras(N_CAM, seed=0).numpy()
    return {"K": Kf, "D": Df, "u": u, "images": images, "masks": masks, "c2w": c2w}


@pytest.fixture(scope="module")
def gpu6(fx6, dev):
    from fruitnerf_amd import _kernels as K
    t = {k: torch.from_numpy(v).to(dev) for k, v in fx6.items()}
    # the set-wide pinhole of the image set is deliberately wrong: the _cams entry points must ignore it
    t["iset"] = K.ImageSetArg(t["images"], t["masks"], t["c2w"], 1.0, 1.0, 0.0, 0.0)
    t["cams"] = K.CameraTableArg(t["K"], t["D"])
    t["ids"] = torch.tensor(TRAIN_IDS, device=dev)
    return t


def _poses(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    pose0 = torch.cat([torch.randn(n, 3, generator=g) * 0.02, torch.randn(n, 3, generator=g) * 0.03], dim=1)
    pose0[0, 3:] = 0.0   # one camera below the 1e-4 clamp of the rotation angle
    return pose0


# ---- 1. directions -------------------------------------------------------------------------------------------------------
def test_sample_pixels_cams_matches_the_float64_camera_model(fx6, gpu6, dev):
    """fnr_sample_pixels_cams: origins, camera indices, image and mask exactly, unit directions within 1e-6 (the bar of
    test_hip_matches_camera_golden for directions through the camera chain) of the float64 reference, whose own residual
    is <= 1e-12.  Teeth: the pinhole directions of the same intrinsics are more than 1e-3 off for the distorted cameras."""
    from fruitnerf_amd import _kernels as K
    o, d, cam, image, mask = K.sample_pixels(gpu6["iset"], gpu6["ids"], gpu6["u"], cams=gpu6["cams"])
    torch.cuda.synchronize()
    k, y, x = _pixels(fx6["u"], len(TRAIN_IDS))
    img = np.asarray(TRAIN_IDS)[k]
    dc, res = _camera_dirs64(img, y, x, fx6["K"], fx6["D"])
    print(f"[camera models] float64 reference residual {res:.2e}")
    assert res <= 1e-12
    c2w = fx6["c2w"].astype(np.float64)[img]
    ref = _world_dirs64(c2w, dc)
    assert torch.equal(o.cpu(), torch.from_numpy(fx6["c2w"][img][:, :, 3]))
    assert torch.equal(cam.cpu(), torch.from_numpy(k.astype(np.int32)))
    assert torch.equal(image.cpu(), torch.from_numpy(fx6["images"][img, y, x]).float() / 255.0)
    assert torch.equal(mask.cpu(), torch.from_numpy(fx6["masks"][img, y, x]).float())
    err = float(np.abs(d.cpu().numpy().astype(np.float64) - ref).max())
    print(f"[camera models] directions: max |hip - float64| {err:.3e}")
    assert err <= 1e-6
    # teeth: what the pinhole formula would have given
    pin = _world_dirs64(c2w, _camera_dirs64(img, y, x, fx6["K"], fx6["D"], undistort=False)[0])
    off = np.abs(pin - ref).max(axis=-1)
    print(f"[camera models] pinhole directions off by up to {off.max():.3e}")
    for i in TRAIN_IDS[1:]:
        assert off[img == i].max() > 1e-3, f"camera {i}: distortion does not show"
    assert off[img == 0].max() <= 1e-12


# ---- 2. zero distortion --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zeros", [False, True])
def test_zero_distortion_is_the_pinhole_path(fx6, gpu6, dev, zeros):
    """A table whose rows repeat one (fx, fy, cx, cy), without distortion (NULL) and with an all-zero one:
    fnr_sample_pixels_cams is fnr_sample_pixels bit for bit, with and without c2w_adjusted."""
    from fruitnerf_amd import _kernels as K
    pin = (43.25, 41.5, 21.3, 22.9)
    iset = K.ImageSetArg(gpu6["images"], gpu6["masks"], gpu6["c2w"], *pin)
    table = K.CameraTableArg(torch.tensor([pin] * N_CAM, device=dev),
                             torch.zeros(N_CAM, 6, device=dev) if zeros else None)
    adj = K.camera_adjust(iset, gpu6["ids"], _poses(len(TRAIN_IDS)).to(dev))
    for c2w_adj in (None, adj):
        ref = K.sample_pixels(iset, gpu6["ids"], gpu6["u"], c2w_adj)
        got = K.sample_pixels(iset, gpu6["ids"], gpu6["u"], c2w_adj, cams=table)
        for name, a, b in zip(("origins", "directions", "cam", "image", "mask"), got, ref):
            assert torch.equal(a, b), name


# ---- 3. prologue ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pose", [True, False])
def test_train_prologue_cams_is_the_separate_launches(gpu6, dev, with_pose):
    """Given the u and jitter it drew, every output of fnr_train_prologue_cams is bit-identical to fnr_camera_adjust +
    fnr_sample_pixels_cams + fnr_sample_spaced (what test_gpu_properties.py asserts for the pinhole prologue)."""
    from fruitnerf_amd import _kernels as K
    S0 = 64
    pose = _poses(len(TRAIN_IDS)).to(dev) if with_pose else None
    out = K.train_prologue(gpu6["iset"], gpu6["ids"], R, seed=1234, offset=7, pose_adjustment=pose, near=0.05, far=1000.0,
                           S0=S0, cams=gpu6["cams"])
    c2w_adj = K.camera_adjust(gpu6["iset"], gpu6["ids"], pose) if with_pose else None
    if with_pose:
        assert torch.equal(out["c2w_adjusted"], c2w_adj)
    o, d, cam, image, mask = K.sample_pixels(gpu6["iset"], gpu6["ids"], out["u"], c2w_adj, cams=gpu6["cams"])
    for name, got, ref in (("origins", out["origins"], o), ("directions", out["directions"], d), ("cam", out["cam"], cam),
                           ("image", out["image"], image), ("mask", out["mask"], mask)):
        assert torch.equal(got, ref), name
    rays = K.RaysArg(o, d, torch.full((R, 1), 0.05, device=dev), torch.full((R, 1), 1000.0, device=dev), cam)
    spacing, euclid = K.sample_spaced(rays, 1, S0, out["jitter"][0])
    assert torch.equal(out["spacing"], spacing) and torch.equal(out["euclid"], euclid)
    assert int(torch.unique(out["cam"]).numel()) == len(TRAIN_IDS)


# ---- 4. pose gradient ----------------------------------------------------------------------------------------------------
def _pose_grad64(pose0, c2w_train, dc, k, Go, Gd):
    """float64 autograd of sum(Go * o + Gd * d) through exp_map_SO3xR3 -> multiply -> ray generation."""
    pose = pose0.double().clone().requires_grad_(True)
    t, w = pose[:, :3], pose[:, 3:]
    theta = torch.sqrt(torch.clamp((w * w).sum(-1), min=1e-4))
    f1 = (torch.sin(theta) / theta)[:, None, None]
    f2 = ((1.0 - torch.cos(theta)) / theta ** 2)[:, None, None]
    z = torch.zeros_like(w[:, 0])
    Kx = torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                      torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)
    Rm = torch.eye(3, dtype=torch.float64)[None] + f1 * Kx + f2 * (Kx @ Kx)
    M = torch.from_numpy(c2w_train)
    R1, t1 = M[:, :, :3], M[:, :, 3]
    Ra = R1 @ Rm
    ta = t1 + (R1 @ t[:, :, None])[:, :, 0]
    kk = torch.from_numpy(k)
    v = (Ra[kk] @ torch.from_numpy(dc)[:, :, None])[:, :, 0]
    d = v / torch.clamp(v.norm(dim=-1, keepdim=True), min=1e-12)
    o = ta[kk]
    ((Go.double() * o).sum() + (Gd.double() * d).sum()).backward()
    return pose.grad


def test_camera_pose_grad_cams_against_float64_autograd(fx6, gpu6, dev):
    """fnr_camera_pose_grad_cams within 1e-4 of max |ref| (the bar of the golden pose-gradient test) of float64 autograd
    through exp-map -> multiply -> this file's ray generation; fnr_camera_pose_grad_adam_cams from the same state gives
    pose and both moments equal to _cams + CameraAdam.step(), the gradient left zero."""
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    from fruitnerf_amd.training import camera_backward_and_step
    n = len(TRAIN_IDS)
    pose0 = _poses(n)
    g = torch.Generator().manual_seed(11)
    Go, Gd = torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g)
    k, y, x = _pixels(fx6["u"], n)
    img = np.asarray(TRAIN_IDS)[k]
    dc, res = _camera_dirs64(img, y, x, fx6["K"], fx6["D"])
    assert res <= 1e-12
    g_ref = _pose_grad64(pose0, fx6["c2w"].astype(np.float64)[TRAIN_IDS], dc, k, Go, Gd)

    def setup():
        cam = CameraOptimizerConfig(mode="SO3xR3").setup(n, dev)
        with torch.no_grad():
            cam.pose_adjustment.copy_(pose0.to(dev))
        cam.pose_adjustment.grad.zero_()
        return cam, CameraAdam(cam)
    cam_a, adam_a = setup()
    c2w_adj = cam_a.adjusted_cameras(gpu6["iset"], gpu6["ids"])
    cam_idx = K.sample_pixels(gpu6["iset"], gpu6["ids"], gpu6["u"], c2w_adj, cams=gpu6["cams"])[2]
    Go_d, Gd_d = Go.to(dev), Gd.to(dev)
    K.camera_pose_grad(gpu6["iset"], gpu6["ids"], gpu6["u"], cam_idx, cam_a.pose_adjustment.data, c2w_adj, Go_d, Gd_d,
                       cam_a.pose_adjustment.grad, cams=gpu6["cams"])
    torch.cuda.synchronize()
    g_hip = cam_a.pose_adjustment.grad.cpu().double()
    scale = float(g_ref.abs().max())
    err = float((g_hip - g_ref).abs().max())
    print(f"[camera models] pose grad: max|ref| {scale:.3e} max_err {err:.3e} rel {err / scale:.3e}")
    assert scale > 0 and err <= 1e-4 * scale
    assert float(g_ref[0, 3:].abs().max()) > 0      # the clamped rotation still has a gradient (through K, not theta)
    adam_a.step()
    # the fused launch from the same state
    cam_b, adam_b = setup()
    K.camera_pose_grad_adam(gpu6["iset"], gpu6["ids"], gpu6["u"], cam_idx, c2w_adj, Go_d, Gd_d, cam_b.pose_adjustment.grad,
                            adam_b.fused_step_args(), cams=gpu6["cams"])
    torch.cuda.synchronize()
    assert torch.equal(cam_b.pose_adjustment.data, cam_a.pose_adjustment.data)
    assert torch.equal(adam_b.exp_avg, adam_a.exp_avg) and torch.equal(adam_b.exp_avg_sq, adam_a.exp_avg_sq)
    assert float(cam_b.pose_adjustment.grad.abs().max()) == 0.0
    assert float((cam_a.pose_adjustment.data.cpu() - pose0).abs().max()) > 0


# ---- 5. full-image rays --------------------------------------------------------------------------------------------------
def test_generate_rays_is_sample_pixels_cams_per_pixel(fx6, gpu6, dev):
    """Cameras.generate_rays(i) of a distorted camera equals fnr_sample_pixels_cams on the u that selects each pixel; the
    row blocks [0, 17) and [17, 48) concatenated are the whole image."""
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.cameras.cameras import Cameras
    Kt = gpu6["K"]
    cams = Cameras(gpu6["c2w"], Kt[:, 0], Kt[:, 1], Kt[:, 2], Kt[:, 3], width=W, height=H, distortion_params=gpu6["D"])
    slot = 2
    i = TRAIN_IDS[slot]
    assert float(gpu6["D"][i].abs().max()) > 0
    rb = cams.generate_rays(i)
    assert rb.origins.shape == (H, W, 3) and rb.directions.shape == (H, W, 3) and rb.pixel_area is None
    assert rb.camera_indices.shape == (H, W, 1) and bool((rb.camera_indices == i).all())
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    u = torch.stack([torch.full((H * W,), (slot + 0.5) / len(TRAIN_IDS)), (ys.reshape(-1) + 0.5) / H,
                     (xs.reshape(-1) + 0.5) / W], -1).float()
    k, y, x = _pixels(u, len(TRAIN_IDS))
    assert (k == slot).all() and (y == ys.reshape(-1).numpy()).all() and (x == xs.reshape(-1).numpy()).all()
    o, d, *_ = K.sample_pixels(gpu6["iset"], gpu6["ids"], u.to(dev), cams=cams.camera_table(dev))
    assert torch.equal(rb.origins.reshape(-1, 3), o) and torch.equal(rb.directions.reshape(-1, 3), d)
    top, bottom = cams.generate_rays(i, rows=(0, 17)), cams.generate_rays(i, rows=(17, 48))
    assert top.origins.shape == (17, W, 3) and bottom.directions.shape == (31, W, 3)
    assert torch.equal(torch.cat([top.directions, bottom.directions]), rb.directions)
    assert torch.equal(torch.cat([top.origins, bottom.origins]), rb.origins)
    assert torch.equal(torch.cat([top.camera_indices, bottom.camera_indices]), rb.camera_indices)


# ---- 6. training through the table ---------------------------------------------------------------------------------------
def _train(dev, cameras_of, steps=24, n_rays=192, n_cam=8, HW=64, focal=90.0):
    """24 TrainingSteps steps of the small model with the camera optimiser on; cameras_of(c2w) -> Cameras | None."""
    import fruitnerf_amd.training as T
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    from fruitnerf_amd.data import synthetic_apple as sa
    scene = sa.make_scene(seed=0, device=dev)
    c2w = sa.make_cameras(n_cam, seed=0, device=dev)
    data = sa.render_dataset(scene, c2w, H=HW, W=HW, fx=focal, fy=focal)
    batcher = sa.PixelBatcher(data, torch.arange(n_cam, device=dev), seed=1, cameras=cameras_of(c2w))
    hm = util.make_hip_like(util.make_oracle(util.small_config(log2=15, prop_log2=13), num_images=n_cam, seed=13), dev)
    hm.train()
    opt = T.FusedAdam(hm)
    cam_opt = CameraOptimizerConfig(mode="SO3xR3").setup(n_cam, dev)
    adam = CameraAdam(cam_opt)
    loop = T.TrainingSteps(hm, opt, batcher, n_rays, camera=(cam_opt, adam))
    for _ in range(steps):
        loop.step()
    torch.cuda.synchronize()
    state = (hm.arena().params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), cam_opt.pose_adjustment.data.clone(),
             adam.exp_avg.clone(), adam.exp_avg_sq.clone())
    return state, dict(loop.stats)


STATE = ("parameters", "exp_avg", "exp_avg_sq", "camera poses", "pose exp_avg", "pose exp_avg_sq")


def test_training_through_an_identity_table_is_training_without(dev):
    """(a) identical rows, zero distortion: parameters, Adam moments and poses equal the run without a table."""
    from fruitnerf_amd.cameras.cameras import Cameras
    HW, focal = 64, 90.0
    with_table, stats = _train(dev, lambda c2w: Cameras(c2w, focal, focal, HW / 2.0, HW / 2.0, width=HW, height=HW,
                                                        distortion_params=torch.zeros(c2w.shape[0], 6)))
    without, _ = _train(dev, lambda c2w: None)
    for name, a, b in zip(STATE, with_table, without):
        assert torch.equal(a, b), name
    assert float(with_table[3].abs().max()) > 0, "the camera optimiser did not move"


def test_training_through_distorted_cameras_replays_as_interpreted(dev):
    """(b) distinct intrinsics and distortion: the replayed run (sequencer on) equals the interpreted run, with
    stats["replayed"] > 0 and no failed recording."""
    import fruitnerf_amd.training as T
    from fruitnerf_amd.cameras.cameras import Cameras
    HW = 64

    def cameras_of(c2w):
        n = c2w.shape[0]
        rng = np.random.default_rng(5)
        fx = torch.tensor(rng.uniform(70, 110, n), dtype=torch.float32)
        dist = torch.tensor(np.stack([rng.uniform(-0.25, 0.15, n), rng.uniform(-0.05, 0.08, n), rng.uniform(-0.01, 0.01, n),
                                      rng.uniform(-0.002, 0.002, n), rng.uniform(-5e-3, 5e-3, n),
                                      rng.uniform(-5e-3, 5e-3, n)], -1), dtype=torch.float32)
        return Cameras(c2w, fx, fx * 1.02, HW / 2.0 + 1.5, HW / 2.0 - 2.0, width=HW, height=HW, distortion_params=dist)
    assert T.NATIVE_SEQUENCER, "the sequencer is the default under test"
    native, stats = _train(dev, cameras_of)
    saved, T.NATIVE_SEQUENCER = T.NATIVE_SEQUENCER, False
    try:
        interpreted, stats_i = _train(dev, cameras_of)
    finally:
        T.NATIVE_SEQUENCER = saved
    print("[camera models] sequencer stats", stats)
    assert stats["replayed"] > 0 and stats["record_failed"] == 0
    assert stats_i["replayed"] == 0
    for name, a, b in zip(STATE, native, interpreted):
        assert torch.equal(a, b), name
    # and the table is in effect: the same loop without it trains to other parameters
    without, _ = _train(dev, lambda c2w: None)
    assert not torch.equal(native[0], without[0])
