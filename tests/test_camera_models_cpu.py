"""CPU: the Python surface of per-image cameras (cameras/cameras.py::Cameras, render_dataset's intrinsics= / distortion=)
and the host-side argument checks of the fnr_*_cams entry points and fnr_camera_rays (no device needed: they return
before any launch)."""
import ctypes as C

import pytest
import torch


def _c2w(n):
    from fruitnerf_amd.data import synthetic_apple as sa
    return sa.make_cameras(n, seed=0)


def test_cameras_fields_per_dataset_and_per_frame():
    from fruitnerf_amd.cameras.cameras import Cameras, PERSPECTIVE
    c2w = _c2w(5)
    per_dataset = Cameras(c2w, 90.0, 91.0, 32.0, 31.0, width=64, height=48)
    assert len(per_dataset) == 5 and per_dataset.width == 64 and per_dataset.height == 48
    for name, v in (("fx", 90.0), ("fy", 91.0), ("cx", 32.0), ("cy", 31.0)):
        col = getattr(per_dataset, name)
        assert col.shape == (5, 1) and col.dtype == torch.float32 and bool((col == v).all())
    assert per_dataset.distortion_params is None and per_dataset.camera_type == PERSPECTIVE
    assert per_dataset.camera_to_worlds.shape == (5, 3, 4)
    fx = torch.linspace(80, 100, 5)
    dist = torch.arange(30, dtype=torch.float64).reshape(5, 6) * 1e-3
    per_frame = Cameras(c2w, fx, fx[:, None] * 1.01, 32.0, torch.full((5,), 30.0), width=64, height=48,
                        distortion_params=dist)
    assert torch.equal(per_frame.fx[:, 0], fx) and per_frame.fy.shape == (5, 1) and per_frame.cy.shape == (5, 1)
    assert per_frame.distortion_params.shape == (5, 6) and per_frame.distortion_params.dtype == torch.float32
    one_row = Cameras(c2w, 90.0, 90.0, 32.0, 24.0, width=64, height=48, distortion_params=dist[1])
    assert one_row.distortion_params.shape == (5, 6) and torch.equal(one_row.distortion_params[4], dist[1].float())
    with pytest.raises(ValueError):
        Cameras(c2w, torch.ones(4), 90.0, 32.0, 24.0, width=64, height=48)
    with pytest.raises(ValueError):
        Cameras(c2w, 90.0, 90.0, 32.0, 24.0, width=64, height=48, distortion_params=torch.zeros(5, 4))
    with pytest.raises(ValueError):
        Cameras(c2w[0], 90.0, 90.0, 32.0, 24.0, width=64, height=48)


def test_only_perspective_cameras():
    from fruitnerf_amd.cameras import cameras as cm
    c2w = _c2w(3)
    for bad in (2, torch.tensor([[1], [2], [1]]), [1, 3, 1]):      # FISHEYE = 2, EQUIRECTANGULAR = 3 in nerfstudio
        with pytest.raises(NotImplementedError, match="PERSPECTIVE"):
            cm.Cameras(c2w, 90.0, 90.0, 32.0, 24.0, width=64, height=48, camera_type=bad)
    ok = cm.Cameras(c2w, 90.0, 90.0, 32.0, 24.0, width=64, height=48, camera_type=torch.ones(3, 1, dtype=torch.long))
    ok.camera_type = 2          # a duck-typed camera set of another type is refused where it is used
    with pytest.raises(NotImplementedError):
        cm.camera_table_of(ok, "cpu")
    with pytest.raises(NotImplementedError):
        cm.generate_rays_of(ok, 0)


def test_camera_table_needs_the_device():
    from fruitnerf_amd.cameras.cameras import Cameras
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cams = Cameras(_c2w(2), 90.0, 90.0, 32.0, 24.0, width=64, height=48)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cams.camera_table("cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        cams.generate_rays(0)


def test_render_dataset_defaults_are_unchanged_and_distortion_shows():
    from fruitnerf_amd.data import synthetic_apple as sa
    scene = sa.make_scene(seed=0)
    c2w = _c2w(2)
    HW, focal = 24, 30.0
    data = sa.render_dataset(scene, c2w, H=HW, W=HW, fx=focal, fy=focal)
    assert set(data) == {"images", "masks", "H", "W", "fx", "fy", "cx", "cy", "c2w"}
    # today's bytes: pixel_rays of the set-wide pinhole -> shade_rays -> uint8
    ys, xs = torch.meshgrid(torch.arange(HW), torch.arange(HW), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    for i in range(2):
        o, d = sa.pixel_rays(c2w, torch.full_like(ys, i), ys, xs, focal, focal, HW / 2.0, HW / 2.0)
        rgb, m = sa.shade_rays(scene, o, d)
        assert torch.equal(data["images"][i], (rgb.view(HW, HW, 3) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8))
        assert torch.equal(data["masks"][i], m.view(HW, HW).to(torch.uint8))
    # the same cameras given per image, undistorted: the same picture (the directions agree to rounding)
    intr = torch.tensor([[focal, focal, HW / 2.0, HW / 2.0]] * 2)
    same = sa.render_dataset(scene, c2w, H=HW, W=HW, intrinsics=intr, distortion=torch.zeros(2, 6))
    assert float((same["images"].int() - data["images"].int()).abs().float().mean()) < 0.5
    assert torch.equal(same["intrinsics"], intr) and same["distortion"].shape == (2, 6)
    # distorted: another picture
    dist = torch.tensor([[-0.2, 0.05, 0.0, 0.0, 3e-3, -2e-3]] * 2)
    bent = sa.render_dataset(scene, c2w, H=HW, W=HW, fx=focal, fy=focal, distortion=dist)
    assert not torch.equal(bent["images"], data["images"])
    assert float((bent["images"].int() - data["images"].int()).abs().float().mean()) > 1.0
    assert torch.equal(bent["intrinsics"], intr)


def test_undistort_inverts_the_opencv_forward_model():
    """data/synthetic_apple.py::undistort_opencv (the contract restated in torch) in float64: forward(undistort(p)) = p."""
    from fruitnerf_amd.data import synthetic_apple as sa
    g = torch.Generator().manual_seed(0)
    p = (torch.rand(500, 2, generator=g, dtype=torch.float64) - 0.5) * 1.6
    D = torch.tensor([-0.2, 0.06, -0.008, 0.002, 4e-3, -5e-3], dtype=torch.float64)
    x, y = sa.undistort_opencv(p[:, 0], p[:, 1], D)
    k1, k2, k3, k4, p1, p2 = D
    r = x * x + y * y
    d = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    fx = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x)
    fy = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y)
    assert float((fx - p[:, 0]).abs().max()) < 1e-12 and float((fy - p[:, 1]).abs().max()) < 1e-12
    assert float((x - p[:, 0]).abs().max()) > 1e-2
    zx, zy = sa.undistort_opencv(p[:, 0].float(), p[:, 1].float(), torch.zeros(6))
    assert torch.equal(zx, p[:, 0].float()) and torch.equal(zy, p[:, 1].float())


def test_null_camera_tables_are_rejected_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    iset = L.fnr_image_set(1, 4, 4, 1, 1, 1, 1.0, 1.0, 0.0, 0.0)       # never dereferenced: the table is checked first
    adam = L.table_adam(0, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 1, 1, 1, None)
    empty = L.fnr_camera_table(None, None)
    p = 1                                                               # a non-null pointer nobody reads
    for cams in (None, C.byref(empty)):
        rc = lib.fnr_sample_pixels_cams(C.byref(iset), cams, p, 1, 16, p, None, p, p, p, p, p, None)
        assert rc == -1 and b"sample_pixels_cams: null camera table" in lib.fnr_last_error()
        rc = lib.fnr_train_prologue_cams(C.byref(iset), cams, p, 1, 16, 0, 0, None, None, p, p, 3, p, p, p, p, p, 0.05,
                                         1000.0, 1, 8, p, p, p, None)
        assert rc == -1 and b"train_prologue_cams: null camera table" in lib.fnr_last_error()
        rc = lib.fnr_camera_pose_grad_cams(C.byref(iset), cams, p, 1, 16, p, p, p, p, p, p, p, None)
        assert rc == -1 and b"camera_pose_grad_cams: null camera table" in lib.fnr_last_error()
        rc = lib.fnr_camera_pose_grad_adam_cams(C.byref(iset), cams, p, 1, 16, p, p, p, p, p, p, C.byref(adam), None)
        assert rc == -1 and b"camera_pose_grad_adam_cams: null camera table" in lib.fnr_last_error()
    # the existing checks still come before any launch
    table = L.fnr_camera_table(p, None)
    rc = lib.fnr_sample_pixels_cams(C.byref(iset), C.byref(table), None, 1, 16, p, None, p, p, p, p, p, None)
    assert rc == -1 and b"null argument" in lib.fnr_last_error()
    rc = lib.fnr_camera_rays(p, None, None, 4, 4, 0, 4, p, p, None)
    assert rc == -1 and b"camera_rays: null argument" in lib.fnr_last_error()
    rc = lib.fnr_camera_rays(p, p, None, 4, 4, 3, 5, p, p, None)
    assert rc == -1 and b"rows [3, 5)" in lib.fnr_last_error()
    assert lib.fnr_camera_rays(p, p, None, 4, 4, 2, 2, p, p, None) == 0   # an empty row block launches nothing
    assert C.sizeof(L.fnr_camera_table) == 16
