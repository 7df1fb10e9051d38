"""CPU side of the camera optimiser's SE3 mode and of odd camera counts: the float64 reference of nerfstudio 0.3.2's
lie_groups.exp_map_SE3 (a restatement, like oracle/camera_opt.py for SO3xR3) pinned on the published definition — the
matrix exponential of the 4 x 4 twist — and what the host layers accept and refuse without a device.
tests/test_gpu_camera_se3.py checks the kernels against the reference written HERE.

Pose rows of the parity tests (pose_rows): angular parts of norm exactly 0 (an all-zero row), 1e-3, 5e-3, 0.012, 0.05,
0.3, 1.0 and 2.5 in random directions, linear parts 0.1 * randn.  No row lies within 20 % of the 1e-2 threshold between the
near-zero polynomials and the closed forms, so float32 and float64 take the same branch."""
import ctypes as C

import torch

THETAS = (0.0, 1e-3, 5e-3, 0.012, 0.05, 0.3, 1.0, 2.5)
NEAR = 1e-2          # theta below: the library's near-zero polynomials


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def skew(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def exp_map_SE3(tv):
    """[N,6] (v, w) -> [N,3,4] = [R | t] in the dtype of tv; differentiable everywhere, the all-zero row included (each
    branch is evaluated in its own variable on values where it is finite, torch.where selects)."""
    v, w = tv[:, :3], tv[:, 3:]
    s = (w * w).sum(-1)
    near = s.detach().sqrt() < NEAR
    th = torch.where(near, torch.ones_like(s), s).sqrt()      # the closed forms never see a small angle
    c_near = 8.0 / (4.0 + s) - 1.0
    ar_near = 0.5 * c_near + 0.5
    c = torch.where(near, c_near, torch.cos(th))
    ar = torch.where(near, ar_near, torch.sin(th) / th)
    br = torch.where(near, 0.5 * ar_near, (1.0 - torch.cos(th)) / th ** 2)
    at = torch.where(near, 1.0 - s / 6.0, torch.sin(th) / th)
    bt = torch.where(near, 0.5 - s / 24.0, (1.0 - torch.cos(th)) / th ** 2)
    ct = torch.where(near, 1.0 / 6.0 - s / 120.0, (th - torch.sin(th)) / th ** 3)
    eye = torch.eye(3, dtype=tv.dtype)[None]
    R = c[:, None, None] * eye + br[:, None, None] * (w[:, :, None] * w[:, None, :]) + ar[:, None, None] * skew(w)
    t = at[:, None] * v + bt[:, None] * torch.linalg.cross(w, v) + ct[:, None] * w * (w * v).sum(-1, keepdim=True)
    return torch.cat([R, t[:, :, None]], -1)


def exp_map_SO3xR3(tv):
    """oracle/camera_opt.py's map restated for float64 autograd (theta clamped at 1e-2, translation = tv[:3])."""
    v, w = tv[:, :3], tv[:, 3:]
    th = torch.sqrt(torch.clamp((w * w).sum(-1), min=1e-4))
    Kx = skew(w)
    R = torch.eye(3, dtype=tv.dtype)[None] + (torch.sin(th) / th)[:, None, None] * Kx \
        + ((1.0 - torch.cos(th)) / th ** 2)[:, None, None] * (Kx @ Kx)
    return torch.cat([R, v[:, :, None]], -1)


def multiply(c2w, delta):
    """pose_utils.multiply: R' = R1 R, t' = t1 + R1 t on [N,3,4]."""
    R1, t1 = c2w[:, :, :3], c2w[:, :, 3]
    return torch.cat([R1 @ delta[:, :, :3], (t1 + (R1 @ delta[:, :, 3:])[:, :, 0])[:, :, None]], -1)


def pose_rows(n=len(THETAS), seed=3, thetas=THETAS):
    """float32 [n,6]: row k has an angular part of norm thetas[k] (up to float32 rounding) and a linear part 0.1 * randn;
    the theta = 0 row is all zero."""
    g = torch.Generator().manual_seed(seed)
    v = 0.1 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    th = torch.tensor(thetas[:n], dtype=torch.float64)
    w = d / d.norm(dim=-1, keepdim=True) * th[:, None]
    rows = torch.cat([v, w], -1)
    rows[th == 0] = 0.0
    return rows.float()


def _matrix_exp(tv):
    X = torch.zeros(tv.shape[0], 4, 4, dtype=tv.dtype)
    X[:, :3, :3] = skew(tv[:, 3:])
    X[:, :3, 3] = tv[:, :3]
    return torch.linalg.matrix_exp(X)[:, :3, :4]


# ---- a. the restatement against the published definition -------------------------------------------------------------------
def test_reference_is_the_matrix_exponential_of_the_twist():
    """Closed forms (theta >= 1e-2) within 1e-12; the near-zero polynomials within 1e-7: the library's a_r differs from
    sin(theta) / theta by theta^2 / 12, i.e. by at most theta^3 / 12 = 8.4e-8 in R below the threshold."""
    rows = torch.cat([pose_rows().double(), pose_rows(3, seed=5, thetas=(9.9e-3, 1.01e-2, 3.1)).double()])
    theta = rows[:, 3:].norm(dim=-1)
    err = (exp_map_SE3(rows) - _matrix_exp(rows)).abs().amax(dim=(1, 2))
    for t, e in zip(theta.tolist(), err.tolist()):
        print(f"[se3 cpu] theta {t:.4e}: max |restatement - matrix_exp| {e:.3e}")
    far = theta >= NEAR
    assert int(far.sum()) >= 6 and int((~far).sum()) >= 4
    assert float(err[far].max()) <= 1e-12
    assert float(err[~far].max()) <= 1e-7
    assert float(err[0]) == 0.0                                 # the all-zero row is the identity exactly
    # the two modes are different maps: same rotation block, another translation
    so3 = exp_map_SO3xR3(rows[far])
    assert float((so3[:, :, :3] - exp_map_SE3(rows[far])[:, :, :3]).abs().max()) <= 1e-12
    assert float((so3[:, :, 3] - exp_map_SE3(rows[far])[:, :, 3]).abs().max()) > 1e-3


def test_reference_gradient_at_the_zero_rotation_is_finite():
    """Autograd at w = 0 (any v): finite, dL/dw = gK + (v x gt) / 2 with gK_i = <dL/dR, K(e_i)>, and dL/dv = gt."""
    g = torch.Generator().manual_seed(0)
    tv = torch.zeros(2, 6, dtype=torch.float64)
    tv[1, :3] = torch.randn(3, generator=g, dtype=torch.float64)
    tv.requires_grad_(True)
    GR = torch.randn(2, 3, 3, generator=g, dtype=torch.float64)
    gt = torch.randn(2, 3, generator=g, dtype=torch.float64)
    out = exp_map_SE3(tv)
    ((GR * out[:, :, :3]).sum() + (gt * out[:, :, 3]).sum()).backward()
    assert bool(torch.isfinite(tv.grad).all())
    gK = torch.stack([GR[:, 2, 1] - GR[:, 1, 2], GR[:, 0, 2] - GR[:, 2, 0], GR[:, 1, 0] - GR[:, 0, 1]], -1)
    want = gK + 0.5 * torch.linalg.cross(tv.detach()[:, :3], gt)
    assert float((tv.grad[:, 3:] - want).abs().max()) <= 1e-14
    assert float((tv.grad[:, :3] - gt).abs().max()) <= 1e-14


# ---- b. the host layers ----------------------------------------------------------------------------------------------------
def test_se3_mode_and_odd_camera_counts_construct():
    from fruitnerf_amd import _lib as L
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    cam = CameraOptimizerConfig(mode="SE3").setup(4, "cpu")
    assert cam.enabled and cam.pose_mode == L.FNR_POSE_SE3 and cam.pose_adjustment.shape == (4, 6)
    assert CameraOptimizerConfig(mode="SO3xR3").setup(4, "cpu").pose_mode == L.FNR_POSE_SO3XR3
    assert CameraOptimizerConfig(mode="off").setup(4, "cpu").get_metrics_dict() == {}
    for mode in ("SO3xR3", "SE3"):
        for algorithm in ("adam", "radam"):
            cam = CameraOptimizerConfig(mode=mode).setup(7, "cpu")
            adam = CameraAdam(cam, algorithm=algorithm)
            assert isinstance(cam.pose_adjustment, torch.nn.Parameter) and cam.pose_adjustment.shape == (7, 6)
            assert cam.pose_adjustment.grad.shape == (7, 6) and adam.exp_avg.shape == adam.exp_avg_sq.shape == (7, 6)
            assert list(cam.state_dict()) == ["pose_adjustment"] and cam.state_dict()["pose_adjustment"].shape == (7, 6)
            assert list(cam.get_param_groups()) == ["camera_opt"]
            # the storages behind the [7,6] views are padded to 44 floats, zero
            for t in (cam.pose_adjustment.data, cam.pose_adjustment.grad, adam.exp_avg, adam.exp_avg_sq):
                assert t.untyped_storage().nbytes() == 4 * 44 and t.is_contiguous()
            # loading a checkpoint keeps the padded storage
            ptr = cam.pose_adjustment.data_ptr()
            cam.load_state_dict({"pose_adjustment": torch.ones(7, 6)})
            assert cam.pose_adjustment.data_ptr() == ptr and float(cam.pose_adjustment.data.sum()) == 42.0
    m = CameraOptimizerConfig(mode="SE3").setup(3, "cpu")
    with torch.no_grad():
        m.pose_adjustment.copy_(torch.arange(18.0).view(3, 6))
    md = m.get_metrics_dict()
    assert sorted(md) == ["camera_opt_rotation", "camera_opt_translation"]
    assert float(md["camera_opt_translation"]) == float(m.pose_adjustment[:, :3].norm())
    assert float(md["camera_opt_rotation"]) == float(m.pose_adjustment[:, 3:].norm())


def test_mode_entry_points_are_declared_and_check_the_mode_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    names = ("fnr_camera_adjust_mode", "fnr_train_prologue_mode", "fnr_camera_pose_grad_mode",
             "fnr_camera_pose_grad_adam_mode")
    for name in names:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert (L.FNR_POSE_SO3XR3, L.FNR_POSE_SE3) == (0, 1) and lib.fnr_abi_version() == 13
    iset = L.fnr_image_set(1, 4, 4, 1, 1, 1, 1.0, 1.0, 0.0, 0.0)       # never dereferenced: the mode is checked first
    adam = L.table_adam(0, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 1, 1, 1, None)
    table = L.fnr_camera_table(1, None)
    p = 1                                                               # a non-null pointer nobody reads
    for cams in (None, C.byref(table)):
        for bad in (2, -1):
            rc = lib.fnr_camera_adjust_mode(p, p, 1, p, bad, p, None)
            assert rc == -1 and b"camera_adjust: pose_mode" in lib.fnr_last_error()
            rc = lib.fnr_train_prologue_mode(C.byref(iset), cams, bad, p, 1, 16, 0, 0, p, p, p, p, 3, p, p, p, p, p, 0.05,
                                             1000.0, 1, 8, p, p, p, None)
            assert rc == -1 and b"train_prologue: pose_mode" in lib.fnr_last_error()
            rc = lib.fnr_camera_pose_grad_mode(C.byref(iset), cams, bad, p, 1, 16, p, p, p, p, p, p, p, None)
            assert rc == -1 and b"camera_pose_grad: pose_mode" in lib.fnr_last_error()
            rc = lib.fnr_camera_pose_grad_adam_mode(C.byref(iset), cams, bad, p, 1, 16, p, p, p, p, p, p, C.byref(adam), None)
            assert rc == -1 and b"camera_pose_grad_adam: pose_mode" in lib.fnr_last_error()
    # a table without intrinsics is refused like in the _cams entry points, in either mode
    empty = L.fnr_camera_table(None, None)
    for mode in (L.FNR_POSE_SO3XR3, L.FNR_POSE_SE3):
        rc = lib.fnr_camera_pose_grad_mode(C.byref(iset), C.byref(empty), mode, p, 1, 16, p, p, p, p, p, p, p, None)
        assert rc == -1 and b"null camera table" in lib.fnr_last_error()
        rc = lib.fnr_camera_adjust_mode(p, None, 1, p, mode, p, None)
        assert rc == -1 and b"null argument" in lib.fnr_last_error()
