"""The camera optimiser's SE3 mode on the device (camera_math.hpp::se3_exp / se3_exp_bwd behind the fnr_*_mode entry points)
and odd camera counts, against the float64 reference of tests/test_camera_se3_cpu.py (nerfstudio 0.3.2's exp_map_SE3
restated and pinned on the matrix exponential there).

Fixture: 8 cameras of 48 x 64 (H x W) on the unit sphere, intrinsics and OpenCV distortion rows drawn like
tests/test_gpu_camera_models.py draws them (focal lengths scaled with the image width, so that the distortion model stays
invertible over the image and the float64 reference converges), u [256, 3].  Pose rows (test_camera_se3_cpu.pose_rows): angular norms 0 (an
all-zero row), 1e-3, 5e-3, 0.012, 0.05, 0.3, 1.0, 2.5, linear parts 0.1 * randn; with 7 cameras the first seven."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util
from tests.test_camera_se3_cpu import exp_map_SE3, exp_map_SO3xR3, multiply, pose_rows
from tests.test_gpu_camera_models import _camera_dirs64, _pixels

pytestmark = pytest.mark.gpu

N_CAM, H, W, R = 8, 48, 64, 256
PIN = (61.5, 59.25, 31.3, 24.9)       # the image set's own pinhole (fx, fy, cx, cy)
SE3, SO3XR3 = 1, 0


@pytest.fixture(scope="module")
def fx8():
    from fruitnerf_amd.data import synthetic_apple as sa
    rng = np.random.default_rng(0)
    fx = rng.uniform(45, 112, N_CAM)     # (that file's 28 .. 70 for W = 40, scaled to W = 64: the same field of view)
    fy = fx * rng.uniform(0.95, 1.05, N_CAM)
    cx = W / 2.0 + rng.uniform(-3, 3, N_CAM)
    cy = H / 2.0 + rng.uniform(-3, 3, N_CAM)
    Df = np.stack([rng.uniform(-0.25, 0.15, N_CAM), rng.uniform(-0.05, 0.08, N_CAM), rng.uniform(-0.01, 0.01, N_CAM),
                   rng.uniform(-0.002, 0.002, N_CAM), rng.uniform(-5e-3, 5e-3, N_CAM), rng.uniform(-5e-3, 5e-3, N_CAM)],
                  -1).astype(np.float32)
    Kf = np.stack([fx, fy, cx, cy], -1).astype(np.float32)
    u = rng.uniform(0, 1, (R, 3)).astype(np.float32)
    u[0], u[1] = 0.999999, 0.0
    images = rng.integers(0, 256, (N_CAM, H, W, 3)).astype(np.uint8)
    masks = rng.integers(0, 2, (N_CAM, H, W)).astype(np.uint8)
    c2w = sa.make_cameras(N_CAM, seed=0).numpy()
    assert np.abs(np.linalg.norm(c2w[:, :, 3], axis=-1) - 1.0).max() < 1e-6      # cameras at unit distance
    g = torch.Generator().manual_seed(11)
    return {"K": Kf, "D": Df, "u": u, "images": images, "masks": masks, "c2w": c2w,
            "Go": torch.randn(R, 3, generator=g).numpy(), "Gd": torch.randn(R, 3, generator=g).numpy()}


@pytest.fixture(scope="module")
def gpu8(fx8, dev):
    from fruitnerf_amd import _kernels as K
    t = {k: torch.from_numpy(v).to(dev) for k, v in fx8.items()}
    t["iset"] = K.ImageSetArg(t["images"], t["masks"], t["c2w"], *PIN)
    t["cams"] = K.CameraTableArg(t["K"], t["D"])
    return t


def _ids(n, dev=None):
    """Training slots -> dataset images: all eight, or seven of them out of order."""
    ids = list(range(N_CAM)) if n == N_CAM else [0, 2, 1, 3, 4, 6, 7]
    return ids if dev is None else torch.tensor(ids, device=dev)


# ---- 1. adjust -------------------------------------------------------------------------------------------------------------
def test_se3_adjust_matches_the_float64_reference(fx8, gpu8, dev):
    """fnr_camera_adjust_mode(SE3) within 1e-6 (the bar of the SO3xR3 ray test) of multiply(c2w, exp_map_SE3(pose)) in
    float64; the all-zero row returns its camera bit for bit; the SO3xR3 adjust of the same rows is another result."""
    from fruitnerf_amd import _kernels as K
    pose = pose_rows()
    ids = _ids(N_CAM, dev)
    got = K.camera_adjust(gpu8["iset"], ids, pose.to(dev), pose_mode=SE3)
    torch.cuda.synchronize()
    ref = multiply(torch.from_numpy(fx8["c2w"]).double(), exp_map_SE3(pose.double()))
    err = (got.cpu().double() - ref).abs().amax(dim=(1, 2))
    print("[se3] adjust: max |hip - float64| per row", " ".join(f"{e:.2e}" for e in err.tolist()))
    assert float(err.max()) <= 1e-6
    assert float(pose[0].abs().max()) == 0.0 and torch.equal(got[0], gpu8["c2w"][0])
    so3 = K.camera_adjust(gpu8["iset"], ids, pose.to(dev))
    assert float((so3 - got)[:, :, 3].abs().max()) > 1e-3
    # CameraOptimizer.forward(): the corrections themselves (identity cameras)
    from fruitnerf_amd.cameras.camera_optimizers import CameraOptimizerConfig
    cam = CameraOptimizerConfig(mode="SE3").setup(N_CAM, dev)
    with torch.no_grad():
        cam.pose_adjustment.copy_(pose.to(dev))
    delta = cam(torch.tensor([7, 0, 3], device=dev))
    assert float((delta.cpu().double() - exp_map_SE3(pose.double())[[7, 0, 3]]).abs().max()) <= 1e-6
    assert torch.equal(cam.adjusted_cameras(gpu8["iset"], ids), got)


# ---- 2. prologue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
def test_se3_prologue_is_the_separate_launches(gpu8, dev, table):
    from fruitnerf_amd import _kernels as K
    cams = gpu8["cams"] if table else None
    ids = _ids(N_CAM, dev)
    pose = pose_rows().to(dev)
    out = K.train_prologue(gpu8["iset"], ids, R, seed=1234, offset=7, pose_adjustment=pose, near=0.05, far=1000.0, S0=16,
                           cams=cams, pose_mode=SE3)
    adj = K.camera_adjust(gpu8["iset"], ids, pose, pose_mode=SE3)
    assert torch.equal(out["c2w_adjusted"], adj)
    o, d, cam, image, mask = K.sample_pixels(gpu8["iset"], ids, out["u"], adj, cams=cams)
    for name, got, ref in (("origins", out["origins"], o), ("directions", out["directions"], d), ("cam", out["cam"], cam),
                           ("image", out["image"], image), ("mask", out["mask"], mask)):
        assert torch.equal(got, ref), name
    assert int(torch.unique(out["cam"]).numel()) == N_CAM
    so3 = K.train_prologue(gpu8["iset"], ids, R, seed=1234, offset=7, pose_adjustment=pose, near=0.05, far=1000.0, S0=16,
                           cams=cams)
    assert torch.equal(so3["u"], out["u"]) and not torch.equal(so3["origins"], out["origins"])


# ---- 3. pose gradient --------------------------------------------------------------------------------------------------------
def _pose_grad64(exp_map, pose0, c2w_train, dc, k, Go, Gd):
    """float64 autograd of sum(Go * o + Gd * d) through exp_map -> multiply -> ray generation."""
    pose = pose0.double().clone().requires_grad_(True)
    Ma = multiply(torch.from_numpy(c2w_train), exp_map(pose))
    kk = torch.from_numpy(k)
    v = (Ma[kk][:, :, :3] @ torch.from_numpy(dc)[:, :, None])[:, :, 0]
    d = v / torch.clamp(v.norm(dim=-1, keepdim=True), min=1e-12)
    o = Ma[kk][:, :, 3]
    ((torch.from_numpy(Go).double() * o).sum() + (torch.from_numpy(Gd).double() * d).sum()).backward()
    return pose.grad


def _rays64(fx8, n, table):
    """(slot per ray, float64 camera-frame directions) of the fixture's u for n training cameras."""
    k, y, x = _pixels(fx8["u"], n, H, W)
    img = np.asarray(_ids(n))[k]
    if table:
        dc, res = _camera_dirs64(img, y, x, fx8["K"], fx8["D"])
        assert res <= 1e-12
    else:
        dc, _ = _camera_dirs64(img, y, x, np.asarray([PIN] * N_CAM, dtype=np.float32), np.zeros((N_CAM, 6), np.float32),
                               undistort=False)
    return k, dc


@pytest.mark.parametrize("n", [8, 7])
@pytest.mark.parametrize("table", [False, True])
def test_se3_pose_grad_against_float64_autograd(fx8, gpu8, dev, table, n):
    """fnr_camera_pose_grad_mode(SE3): translation and rotation columns each within 1e-4 of their max |ref| (the
    project's pose-gradient bar), no NaN, a gradient on the all-zero row's rotation; the SO3xR3 reference of the same
    inputs is more than 10 tolerances away in the translation columns, so a kernel that ignores the mode fails."""
    from fruitnerf_amd import _kernels as K
    cams = gpu8["cams"] if table else None
    ids = _ids(n, dev)
    pose0 = pose_rows(n)
    k, dc = _rays64(fx8, n, table)
    c2w_train = fx8["c2w"].astype(np.float64)[_ids(n)]
    g_ref = _pose_grad64(exp_map_SE3, pose0, c2w_train, dc, k, fx8["Go"], fx8["Gd"])
    g_so3 = _pose_grad64(exp_map_SO3xR3, pose0, c2w_train, dc, k, fx8["Go"], fx8["Gd"])
    pose = pose0.to(dev)
    adj = K.camera_adjust(gpu8["iset"], ids, pose, pose_mode=SE3)
    cam_idx = K.sample_pixels(gpu8["iset"], ids, gpu8["u"], adj, cams=cams)[2]
    assert np.array_equal(cam_idx.cpu().numpy(), k.astype(np.int32))
    grad = torch.zeros(n, 6, device=dev)
    K.camera_pose_grad(gpu8["iset"], ids, gpu8["u"], cam_idx, pose, adj, gpu8["Go"], gpu8["Gd"], grad, cams=cams,
                       pose_mode=SE3)
    torch.cuda.synchronize()
    g_hip = grad.cpu().double()
    assert bool(torch.isfinite(g_hip).all())
    tol = 1e-4
    for name, cols in (("translation", slice(0, 3)), ("rotation", slice(3, 6))):
        scale = float(g_ref[:, cols].abs().max())
        err = float((g_hip[:, cols] - g_ref[:, cols]).abs().max())
        print(f"[se3] pose grad ({'table' if table else 'pinhole'}, n={n}) {name}: max|ref| {scale:.3e} max_err {err:.3e} "
              f"rel {err / scale:.3e}")
        assert scale > 0 and err <= tol * scale, name
    assert float(g_hip[0, 3:].abs().max()) > 0 and float(pose0[0].abs().max()) == 0.0
    t_scale = float(g_ref[:, :3].abs().max())
    apart = float((g_ref[:, :3] - g_so3[:, :3]).abs().max())
    print(f"[se3] SE3 vs SO3xR3 reference, translation columns: {apart / t_scale:.3e} of max|ref|")
    assert apart > 10 * tol * t_scale


# ---- 4. fused = unfused ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["adam", "radam"])
def test_se3_fused_gradient_and_step_is_gradient_then_step(gpu8, dev, algorithm):
    """fnr_camera_pose_grad_adam_mode(SE3) from the same state = fnr_camera_pose_grad_mode + CameraAdam.step(), bit for
    bit, with the gradient left zero; 7 cameras, through the camera table."""
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    n = 7
    ids = _ids(n, dev)
    pose0 = pose_rows(n).to(dev)

    def setup():
        cam = CameraOptimizerConfig(mode="SE3").setup(n, dev)
        with torch.no_grad():
            cam.pose_adjustment.copy_(pose0)
        return cam, CameraAdam(cam, algorithm=algorithm)
    cam_a, adam_a = setup()
    adj = cam_a.adjusted_cameras(gpu8["iset"], ids)
    cam_idx = K.sample_pixels(gpu8["iset"], ids, gpu8["u"], adj, cams=gpu8["cams"])[2]
    K.camera_pose_grad(gpu8["iset"], ids, gpu8["u"], cam_idx, cam_a.pose_adjustment.data, adj, gpu8["Go"], gpu8["Gd"],
                       cam_a.pose_adjustment.grad, cams=gpu8["cams"], pose_mode=cam_a.pose_mode)
    assert float(cam_a.pose_adjustment.grad.abs().min()) > 0
    adam_a.step()
    cam_b, adam_b = setup()
    K.camera_pose_grad_adam(gpu8["iset"], ids, gpu8["u"], cam_idx, adj, gpu8["Go"], gpu8["Gd"], cam_b.pose_adjustment.grad,
                            adam_b.fused_step_args(), cams=gpu8["cams"], pose_mode=cam_b.pose_mode)
    torch.cuda.synchronize()
    assert torch.equal(cam_b.pose_adjustment.data, cam_a.pose_adjustment.data)
    assert torch.equal(adam_b.exp_avg, adam_a.exp_avg) and torch.equal(adam_b.exp_avg_sq, adam_a.exp_avg_sq)
    assert float(cam_b.pose_adjustment.grad.abs().max()) == 0.0 and float(cam_a.pose_adjustment.grad.abs().max()) == 0.0
    assert float((cam_a.pose_adjustment.data - pose0).abs().max()) > 0


# ---- 5. odd counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["adam", "radam"])
def test_odd_camera_count_steps_like_the_prefix_of_the_even_count(dev, algorithm):
    """CameraAdam.step() on 7 cameras = the first 42 entries of the same steps on 8 cameras with the same gradient rows,
    bit for bit, over 3 steps; the two padding lanes behind the 42 floats are still zero."""
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig, _padded_flat
    g = torch.Generator().manual_seed(2)
    pose0 = pose_rows(8).to(dev)
    grads = [torch.randn(8, 6, generator=g).to(dev) for _ in range(3)]

    def run(n):
        cam = CameraOptimizerConfig(mode="SO3xR3").setup(n, dev)
        adam = CameraAdam(cam, algorithm=algorithm)
        with torch.no_grad():
            cam.pose_adjustment.copy_(pose0[:n])
        for gr in grads:
            cam.pose_adjustment.grad.copy_(gr[:n])
            adam.step()
            assert float(cam.pose_adjustment.grad.abs().max()) == 0.0
        torch.cuda.synchronize()
        return cam, adam
    cam7, adam7 = run(7)
    cam8, adam8 = run(8)
    for name, a, b in (("pose", cam7.pose_adjustment.data, cam8.pose_adjustment.data), ("exp_avg", adam7.exp_avg, adam8.exp_avg),
                       ("exp_avg_sq", adam7.exp_avg_sq, adam8.exp_avg_sq)):
        assert a.shape == (7, 6) and torch.equal(a, b[:7]), name
        flat = _padded_flat(a)
        assert flat.numel() == 44 and flat.data_ptr() == a.data_ptr() and float(flat[42:].abs().max()) == 0.0, name
    assert float(_padded_flat(cam7.pose_adjustment.grad)[42:].abs().max()) == 0.0
    assert float((cam7.pose_adjustment.data - pose0[:7]).abs().max()) > 0


# ---- 6. training -------------------------------------------------------------------------------------------------------------
STATE = ("parameters", "exp_avg", "exp_avg_sq", "camera poses", "pose exp_avg", "pose exp_avg_sq")


@pytest.fixture(scope="module")
def scene8(dev):
    from fruitnerf_amd.data import synthetic_apple as sa
    scene = sa.make_scene(seed=0, device=dev)
    c2w = sa.make_cameras(N_CAM, seed=0, device=dev)
    return sa.render_dataset(scene, c2w, H=64, W=64, fx=90.0, fy=90.0)


def _train(dev, data, n_cam=N_CAM, steps=24, n_rays=192, mode="SE3"):
    """24 TrainingSteps steps of the small model on the first n_cam cameras, camera optimiser in `mode`."""
    import fruitnerf_amd.training as T
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    from fruitnerf_amd.data import synthetic_apple as sa
    batcher = sa.PixelBatcher(data, torch.arange(n_cam, device=dev), seed=1)
    hm = util.make_hip_like(util.make_oracle(util.small_config(log2=15, prop_log2=13), num_images=n_cam, seed=13), dev)
    hm.train()
    opt = T.FusedAdam(hm)
    cam_opt = CameraOptimizerConfig(mode=mode).setup(n_cam, dev)
    adam = CameraAdam(cam_opt)
    loop = T.TrainingSteps(hm, opt, batcher, n_rays, camera=(cam_opt, adam))
    for _ in range(steps):
        loop.step()
    torch.cuda.synchronize()
    state = (hm.arena().params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), cam_opt.pose_adjustment.data.clone(),
             adam.exp_avg.clone(), adam.exp_avg_sq.clone())
    return state, dict(loop.stats), cam_opt


def test_se3_training_replays_as_interpreted(dev, scene8):
    """The replayed run (sequencer on) equals the interpreted run and a second replayed run; both pose blocks moved; the
    metrics are the torch norms; the SO3xR3 loop on the same data trains to other poses."""
    import fruitnerf_amd.training as T
    assert T.NATIVE_SEQUENCER, "the sequencer is the default under test"
    native, stats, cam_opt = _train(dev, scene8)
    again, stats2, _ = _train(dev, scene8)
    saved, T.NATIVE_SEQUENCER = T.NATIVE_SEQUENCER, False
    try:
        interpreted, stats_i, _ = _train(dev, scene8)
    finally:
        T.NATIVE_SEQUENCER = saved
    print("[se3] sequencer stats", stats)
    assert stats["replayed"] > 0 and stats["record_failed"] == 0
    assert stats2["replayed"] > 0 and stats2["record_failed"] == 0
    assert stats_i["replayed"] == 0
    for name, a, b, c in zip(STATE, native, interpreted, again):
        assert torch.equal(a, b), name
        assert torch.equal(a, c), name + " (second run)"
    pose = native[3]
    assert bool(torch.isfinite(pose).all())
    assert float(pose[:, :3].abs().max()) > 0 and float(pose[:, 3:].abs().max()) > 0
    md = cam_opt.get_metrics_dict()
    assert sorted(md) == ["camera_opt_rotation", "camera_opt_translation"] and md["camera_opt_rotation"].device.type == "cuda"
    assert torch.equal(md["camera_opt_translation"], pose[:, :3].norm())
    assert torch.equal(md["camera_opt_rotation"], pose[:, 3:].norm())
    so3, _, _ = _train(dev, scene8, mode="SO3xR3")
    assert not torch.equal(so3[3], pose)


def test_se3_training_with_seven_cameras(dev, scene8):
    state, stats, cam_opt = _train(dev, scene8, n_cam=7)
    pose = state[3]
    assert pose.shape == (7, 6) and bool(torch.isfinite(pose).all())
    assert float(pose[:, :3].abs().max()) > 0 and float(pose[:, 3:].abs().max()) > 0
    assert stats["record_failed"] == 0


# ---- 7. SO3xR3 through the new entry points ------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
def test_mode_entry_points_with_so3xr3_are_the_old_entry_points(gpu8, dev, table):
    """pose_mode = FNR_POSE_SO3XR3: every output of the four fnr_*_mode symbols equals that of the symbols without a mode."""
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd import _lib as L
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    lib = L.load()
    iset, cams = gpu8["iset"], (gpu8["cams"] if table else None)
    cref = None if cams is None else cams.ref(iset)
    n = 7
    ids = _ids(n, dev)
    pose = pose_rows(n).to(dev)
    stream = L.stream_ptr(dev)
    # adjust
    adj = K.camera_adjust(iset, ids, pose)
    adj_m = torch.empty_like(adj)
    L.check(lib.fnr_camera_adjust_mode(L.ptr(iset.c2w), L.ptr(ids), n, L.ptr(pose), SO3XR3, L.ptr(adj_m), stream), "adjust")
    assert torch.equal(adj_m, adj)
    # prologue
    S0 = 16
    old = K.train_prologue(iset, ids, R, seed=99, offset=3, pose_adjustment=pose, near=0.05, far=1000.0, S0=S0, cams=cams)
    new = {k: (torch.full_like(v, -7) if torch.is_tensor(v) else v) for k, v in old.items()}
    base = K.host_linspace(0.0, 1.0, S0 + 1, dev)
    L.check(lib.fnr_train_prologue_mode(C.byref(iset.c), cref, SO3XR3, L.ptr(ids), n, R, 99, 3, L.ptr(pose),
                                        L.ptr(new["c2w_adjusted"]), L.ptr(new["u"]), L.ptr(new["jitter"]), 3,
                                        L.ptr(new["origins"]), L.ptr(new["directions"]), L.ptr(new["cam"]), L.ptr(new["image"]),
                                        L.ptr(new["mask"]), 0.05, 1000.0, 1, S0, L.ptr(base), L.ptr(new["spacing"]),
                                        L.ptr(new["euclid"]), stream), "prologue")
    for k, v in old.items():
        if torch.is_tensor(v):
            assert torch.equal(new[k], v), k
    # pose gradient, and gradient + optimiser step
    cam_idx = K.sample_pixels(iset, ids, gpu8["u"], adj, cams=cams)[2]
    g_old, g_new = torch.zeros(n, 6, device=dev), torch.zeros(n, 6, device=dev)
    K.camera_pose_grad(iset, ids, gpu8["u"], cam_idx, pose, adj, gpu8["Go"], gpu8["Gd"], g_old, cams=cams)
    L.check(lib.fnr_camera_pose_grad_mode(C.byref(iset.c), cref, SO3XR3, L.ptr(ids), n, R, L.ptr(gpu8["u"]), L.ptr(cam_idx),
                                          L.ptr(pose), L.ptr(adj), L.ptr(gpu8["Go"]), L.ptr(gpu8["Gd"]), L.ptr(g_new), stream),
            "pose_grad")
    assert torch.equal(g_new, g_old) and float(g_old.abs().max()) > 0

    def setup():
        cam = CameraOptimizerConfig(mode="SO3xR3").setup(n, dev)
        with torch.no_grad():
            cam.pose_adjustment.copy_(pose)
        return cam, CameraAdam(cam)
    cam_a, adam_a = setup()
    K.camera_pose_grad_adam(iset, ids, gpu8["u"], cam_idx, adj, gpu8["Go"], gpu8["Gd"], cam_a.pose_adjustment.grad,
                            adam_a.fused_step_args(), cams=cams)
    cam_b, adam_b = setup()
    args = adam_b.fused_step_args()
    L.check(lib.fnr_camera_pose_grad_adam_mode(C.byref(iset.c), cref, SO3XR3, L.ptr(ids), n, R, L.ptr(gpu8["u"]),
                                               L.ptr(cam_idx), L.ptr(adj), L.ptr(gpu8["Go"]), L.ptr(gpu8["Gd"]),
                                               L.ptr(cam_b.pose_adjustment.grad), C.byref(args), stream), "pose_grad_adam")
    torch.cuda.synchronize()
    assert torch.equal(cam_b.pose_adjustment.data, cam_a.pose_adjustment.data)
    assert torch.equal(adam_b.exp_avg, adam_a.exp_avg) and torch.equal(adam_b.exp_avg_sq, adam_a.exp_avg_sq)
    assert float((cam_a.pose_adjustment.data - pose).abs().max()) > 0
