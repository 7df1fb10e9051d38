"""GPU: analytic normals — fnr_field_normals per sample against the float64 reference of tests/normals_reference.py,
fnr_render_normals, fnr_depth_points_normals, FruitField.get_normals() end to end against float64 autograd through the oracle's
field, the model's "normals" output and generate_point_cloud(normal_method="model_output").

The bound of a kept sample: ||n_got - n_ref||_2 <= C_NORMALS (2 E / ||g|| + 4 u), E the running error estimate of the
gradient (normals_reference's docstring).  Measured worst ratios ||err|| / (2 E / ||g|| + 4 u), over the cases
field_reference.CASES + (33, 48) (no sample is next to a kink of a1 in any of them):
    float32 emulation on the CPU   fruit_nerf 0.0517   fruit_nerf_big 0.0498     -> C_NORMALS = 0.25 (>= 4 x)
    fnr_field_normals on MI355X    fruit_nerf 0.0517   fruit_nerf_big 0.0498     (the chains are the emulation's)
For the record (not bounds): the emulation's worst ||err|| is 2.3e-6, the worst sum |df| |J| / ||g|| 141.
The wrong references (row 1 of W_b1; Jacobian axes 0 and 2 exchanged) miss the bound on every case, N = 1 included.

get_normals end to end (util.small_config / big_config, 64 rays x 48 samples; error = ||n - n_float64||_2 per selected sample,
the samples on which the float32 oracle is off by more than 1e-2 left out; measured on MI355X):
                                  device median / p99     float32 oracle median / p99    left out
    fruit_nerf      contraction   3.00e-05 / 1.90e-04     3.00e-05 / 1.90e-04            2 of 3072
    fruit_nerf      aabb          3.00e-05 / 1.80e-04     3.00e-05 / 1.80e-04            5 of 2632
    fruit_nerf_big  contraction   5.99e-05 / 3.73e-04     5.98e-05 / 3.73e-04            4 of 3072
    fruit_nerf_big  aabb          5.93e-05 / 4.08e-04     5.93e-05 / 4.08e-04            7 of 2632
The float32 oracle is off by more than 1e-4 on 6 % (fruit_nerf) and 27 % (fruit_nerf_big) of the samples: cell and gate flips.
"""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cloud_knn_reference as R_
from tests import field_reference as fr
from tests import normals_reference as nr
from tests import util

pytestmark = pytest.mark.gpu

MODE_ID = {"fp32": 0, "bf16": 1, "bf16x3": 3}


def _K():
    from fruitnerf_amd import _kernels as K
    return K


def _L():
    from fruitnerf_amd import _lib as L
    return L


class _Net:
    """The base MLP of a field_reference network as an fnr_field_net (fnr_field_normals reads nothing else)."""

    def __init__(self, dev, net, mode="fp32"):
        L, K = _L(), _K()
        self.t = [t.to(dev).contiguous() for k in ("base0", "base1") for t in net[k]]
        self._dummy = torch.zeros(64, device=dev)
        n = L.fnr_field_net()
        n.grid = K.make_grid(self._dummy, 16, 4, [16] * 16)
        n.geo_feat_dim, n.hidden_dim = net["geo"], 64
        n.base_w0, n.base_b0, n.base_w1, n.base_b1 = (L.ptr(t) for t in self.t)
        n.mlp_mode = MODE_ID[mode]
        self.c = n


_REF = {}


def _case(shape, R, S):
    key = (shape, R, S)
    if key not in _REF:
        if len(_REF) > 4:
            _REF.clear()
        net, batch, jac = nr.case_inputs(shape, R, S)
        ref = nr.reference(net, batch, jac)
        kink = nr.kink_of_a1(net, batch, ref["f"])
        _REF[key] = dict(net=net, batch=batch, jac=jac, ref=ref, kink=kink)
    return _REF[key]


@pytest.mark.parametrize("R,S", nr.CASES)
@pytest.mark.parametrize("shape", nr.SHAPE_LIST)
def test_field_normals_per_sample(dev, shape, R, S):
    K = _K()
    c = _case(shape, R, S)
    net, batch, jac, ref, kink = c["net"], c["batch"], c["jac"], c["ref"], c["kink"]
    N = batch["N"]
    assert int(kink.sum()) < 0.01 * N
    keep = ~kink
    feats, jd = batch["feats"].to(dev).contiguous(), jac.to(dev).contiguous()
    sel = batch["sel"].to(torch.uint8).to(dev).contiguous()
    got = {}
    for mode in ("fp32", "bf16x3", "bf16"):
        dn = _Net(dev, net, mode)
        n, g = K.field_normals(dn.c, feats, jd, sel, want_gradient=True)
        n_only = K.field_normals(dn.c, feats, jd, sel)
        torch.cuda.synchronize()
        got[mode] = (n.cpu(), g.cpu())
        assert torch.equal(n_only.cpu(), got[mode][0])                       # a second call, without `gradient`: same bits
    for mode in ("bf16x3", "bf16"):
        assert torch.equal(got[mode][0], got["fp32"][0]) and torch.equal(got[mode][1], got["fp32"][1]), mode
    n, g = got["fp32"]
    unsel = ~batch["sel"]
    assert bool((n[unsel] == 0).all()) and bool((g[unsel] == 0).all())
    r = nr.ratios(n, ref, keep)
    gerr = ((g.double() - ref["g"]).norm(dim=1) / ref["E"].clamp_min(1e-300))[keep & batch["sel"]]
    print(f"[normals gpu] {shape} ({R},{S}): worst ||err|| / bound = {float(r.max()):.3g} (C_NORMALS {nr.C_NORMALS}), "
          f"gradient worst ||err|| / E = {float(gerr.max()) if gerr.numel() else 0.0:.3g}")
    assert float(r.max()) <= nr.C_NORMALS
    # teeth: the same check against a wrong reference fails
    for kw in (dict(row=1), dict(swap_axes=(0, 2))):
        wrong = nr.reference(net, batch, jac, **kw)
        assert float(nr.ratios(n, wrong, keep).max()) > nr.C_NORMALS, kw


def test_field_normals_rejects_unbuilt_shapes(dev):
    L = _L()
    net = fr.make_net("fruit_nerf", 0)
    dn = _Net(dev, net)
    dn.c.geo_feat_dim = 16
    t = torch.zeros(16, 3, 4, 2, device=dev)
    rc = L.load().fnr_field_normals(C.byref(dn.c), 4, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), None, None)
    assert rc == -2


@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("S", [1, 48, 129])
def test_render_normals(dev, R, S):
    K = _K()
    g = torch.Generator().manual_seed(1000 * R + S)
    w = torch.rand(R, S, generator=g) / S
    if R > 1:
        w[R // 2] = 0.0                                                     # a ray that hits nothing
    n = torch.nn.functional.normalize(torch.randn(R, S, 3, generator=g), dim=-1)
    for shade in (False, True):
        got = K.render_normals(w.to(dev), n.to(dev).view(-1, 3), S, shade).cpu()
        want = nr.render_reference(w, n, shade)
        # float32: S products and S sums, each within u of a partial sum <= sum w: |dn| <= (S + 1) u sum w, relative to ||n||;
        # normalising at most doubles it; + the squares, their sums, the root, the quotient, the shift and the halving
        tol = (2 * (S + 1) + 6) * fr.U * float((w.double().sum(1) / (w.double()[..., None] * n.double()).sum(1).norm(dim=1).clamp_min(1e-30))
                                     [w.sum(1) > 0].max())
        err = float((got.double() - want).abs().max())
        print(f"[render normals] R {R} S {S} shade {shade}: max |err| {err:.3g} (tolerance {tol:.3g})")
        assert err <= tol
        if R > 1:
            assert bool((got[R // 2] == (0.5 if shade else 0.0)).all())
        again = K.render_normals(w.to(dev), n.to(dev).view(-1, 3), S, shade).cpu()
        assert torch.equal(got, again)


def test_depth_points_normals(dev):
    K = _K()
    R = 5000
    g = torch.Generator().manual_seed(11)
    o = (torch.rand(R, 3, generator=g) - 0.5).to(dev)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(dev)
    t = (torch.rand(R, generator=g) * 0.8).to(dev)
    rgb = torch.rand(R, 3, generator=g).to(dev)
    attr = torch.randn(R, 3, generator=g).to(dev)
    box = ((-10.0, -10.0, -10.0), (0.0, 10.0, 10.0))                         # x < 0: about half of the rays
    cap = 2 * R

    def run(with_attr):
        pts, cols = torch.full((cap, 3), -7.0, device=dev), torch.full((cap, 3), -7.0, device=dev)
        out = torch.full((cap, 3), -7.0, device=dev) if with_attr else None
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        for _ in range(2):                                                  # two consecutive batches
            K.depth_points(o, d, t, rgb, box[0], box[1], pts, cols, cnt, normals=attr if with_attr else None,
                           normals_out=out)
        return pts.cpu(), cols.cpu(), int(cnt.item()), None if out is None else out.cpu()

    p0, c0, n0, _ = run(False)
    p1, c1, n1, a1 = run(True)
    assert n0 == n1 and 0.8 * R < n0 < 1.2 * R
    assert torch.equal(p0, p1) and torch.equal(c0, c1)
    # kept ray i carries row i of the input: the torch restatement of fnr_depth_points with the attribute in rgb's place
    want_p, want_a = R_.depth_points(o, d, t, attr, *box)
    m = n0 // 2
    assert want_p.shape[0] == m and torch.equal(p1[:m], want_p.cpu()) and torch.equal(p1[m:n0], want_p.cpu())
    assert torch.equal(a1[:m], want_a.cpu()) and torch.equal(a1[m:n0], want_a.cpu())
    assert bool((a1[n0:] == -7.0).all())                                    # nothing written past the count


def _field_samples(R, S, dev, seed):
    from fruitnerf_amd.rays import RayBundle
    o, d, pa, cam = util.random_rays(R, 7, seed=seed)
    g = torch.Generator().manual_seed(seed)
    euclid = torch.sort(torch.rand(R, S + 1, generator=g) * 2.4 + 0.1, dim=-1).values
    hb = RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))
    return hb, hb.get_ray_samples(euclid[:, :-1, None].to(dev), euclid[:, 1:, None].to(dev)), euclid


@pytest.mark.parametrize("shape", ["fruit_nerf", "fruit_nerf_big"])
@pytest.mark.parametrize("contract", [True, False], ids=["contraction", "aabb"])
def test_get_normals_end_to_end(dev, contract, shape):
    from fruitnerf_amd.fruit_field import FieldHeadNames
    K = _K()
    cfg = (util.small_config if shape == "fruit_nerf" else util.big_config)()
    cfg.disable_scene_contraction = not contract
    om = util.make_oracle(cfg, seed=7)
    hm = util.make_hip_like(om, dev)
    om.eval()
    hm.eval()
    fld = hm.field
    R, S = 64, 48
    hb, hs, euclid = _field_samples(R, S, dev, seed=9)
    plain = fld(hs)
    with_n = fld(hs, compute_normals=True)
    for k in (FieldHeadNames.DENSITY, FieldHeadNames.RGB, FieldHeadNames.SEMANTICS):
        assert torch.equal(plain[k], with_n[k]), k
    assert set(plain) == {FieldHeadNames.DENSITY, FieldHeadNames.RGB, FieldHeadNames.SEMANTICS}
    normals = fld.get_normals()
    assert normals.shape == (R, S, 3) and not normals.requires_grad
    assert torch.equal(normals, with_n[FieldHeadNames.NORMALS])
    # bit-equal to the two launches by hand (flattened ray samples: one "ray" per sample)
    rays, eu, S1, _ = fld._flatten(hs)
    net = fld.net_struct()
    feats, selector, jac = K.hash_encode_fwd(net.grid, fld.warp_struct(), rays, eu, S1, want_jacobian=True)
    by_hand = K.field_normals(net, feats, jac, selector)
    assert torch.equal(by_hand.view(R, S, 3), normals)
    # structured ray samples (what the model hands out) give the same bits; so does every test_mode / training flag
    hs2 = hb.get_ray_samples(euclid[:, :-1, None].to(dev), euclid[:, 1:, None].to(dev))
    hs2._structured = (K.RaysArg(hb.origins, hb.directions, None, None, hb.camera_indices), euclid.to(dev).contiguous(), S)
    fld.get_density(hs2)
    assert torch.equal(fld.get_normals(), normals)
    for test_mode, training in (("inference", False), ("export", False), (None, True)):
        fld.test_mode = test_mode
        fld.train(training)
        with torch.no_grad():
            fld.get_density(hs)
        assert torch.equal(fld.get_normals(), normals), (test_mode, training)
    fld.test_mode = None
    fld.eval()
    # float64 autograd through a double copy of the oracle's field at the float32 sample locations
    fld.get_density(hs)
    pos = fld._sample_locations.detach().cpu().reshape(-1, 3)
    sel = ((pos > 0) & (pos < 1)).all(1)
    got = normals.cpu().reshape(-1, 3)
    assert bool((got[~sel] == 0).all()) and (contract or int((~sel).sum()) > 0)
    f64 = copy.deepcopy(om.field).double()
    n64, _ = nr.autograd_normals(f64, pos.double())
    n32, _ = nr.autograd_normals(om.field, pos)
    e_dev = (got.double() - n64).norm(dim=1)[sel]
    e_o32 = (n32.double() - n64).norm(dim=1)[sel]
    off = e_o32 > 1e-2
    assert int(off.sum()) <= 0.01 * int(sel.sum())
    e_dev, e_o32 = e_dev[~off], e_o32[~off]
    q = lambda e, p: float(torch.quantile(e, p))   # noqa: E731
    print(f"[get_normals] {shape} contract={contract}: device median {q(e_dev, 0.5):.3g} p99 {q(e_dev, 0.99):.3g}; float32 oracle "
          f"median {q(e_o32, 0.5):.3g} p99 {q(e_o32, 0.99):.3g}; left out {int(off.sum())} of {int(sel.sum())}; "
          f"oracle > 1e-4: {float((e_o32 > 1e-4).double().mean()):.3g}")
    assert q(e_dev, 0.5) <= 2 * q(e_o32, 0.5) and q(e_dev, 0.99) <= 2 * q(e_o32, 0.99)
    fld.release_last_samples()
    with pytest.raises(AttributeError):
        fld.get_normals()
    with pytest.raises(AttributeError):
        fld._sample_locations


def test_model_normals_output(dev):
    from fruitnerf_amd.rays import RayBundle
    om = util.make_oracle(util.small_config(), seed=3)
    hm = util.make_hip_like(om, dev)
    hm.eval()
    H = W = 8
    o, d, pa, cam = util.random_rays(H * W, 7, seed=4)
    flat = RayBundle(o.to(dev), d.to(dev), None, None)
    flat_cam = RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))
    cam_rb = RayBundle(flat.origins.view(H, W, 3), flat.directions.view(H, W, 3), None, None)
    assert hm.config.render_normals is False
    off = hm.get_outputs_for_camera_ray_bundle(cam_rb)
    assert "normals" not in off
    hm.config.render_normals = True
    on = hm.get_outputs_for_camera_ray_bundle(cam_rb)
    assert on["normals"].shape == (H, W, 3) and float(on["normals"].min()) >= 0.0 and float(on["normals"].max()) <= 1.0
    assert float(on["normals"].std()) > 0.01
    assert set(on) == set(off) | {"normals"}
    for k in off:
        assert torch.equal(on[k], off[k]), k
    sharded = hm.get_outputs_for_camera_ray_bundle(cam_rb, rank=0, world_size=1)
    for k in on:
        assert torch.equal(sharded[k], on[k]), k
    # the output is the renderer over the final level's weights of the field's normals of those samples, shaded
    out = hm(flat)
    rs, w = out["ray_samples_list"][-1], out["weights_list"][-1]
    hm.field.get_density(rs)
    want = _K().render_normals(w[..., 0], hm.field.get_normals().reshape(-1, 3), w.shape[1], shade=True)
    assert torch.equal(out["normals"], want) and torch.equal(out["normals"], on["normals"].view(-1, 3))
    # eval images carry it
    g = torch.Generator().manual_seed(0)
    batch = {"image": torch.rand(16, 16, 3, generator=g), "fruit_mask": (torch.rand(16, 16, 1, generator=g) > 0.7).float()}
    o2, d2, _, _ = util.random_rays(256, 7, seed=5)
    big = hm.get_outputs_for_camera_ray_bundle(RayBundle(o2.to(dev).view(16, 16, 3), d2.to(dev).view(16, 16, 3), None, None))
    _, images = hm.get_image_metrics_and_images(big, batch)
    assert torch.equal(images["normals"], big["normals"])
    # 'inference' mode has it too, 'export' mode and training do not
    hm.test_mode = hm.field.test_mode = "inference"
    inf = hm(flat)
    assert inf["normals"].shape == (H * W, 3) and 0.0 <= float(inf["normals"].min()) and float(inf["normals"].max()) <= 1.0
    hm.test_mode = hm.field.test_mode = None
    hm.train()
    assert "normals" not in hm(flat_cam)
    with torch.no_grad():
        assert "normals" not in hm(flat_cam)


class _Shifted:
    """pipeline.model whose "normals" leave [0,1]."""

    def __init__(self, model):
        self.model, self.device = model, model.device

    def __call__(self, ray_bundle):
        out = dict(self.model(ray_bundle))
        out["normals"] = out["rgb"] - 1.0
        return out


def test_generate_point_cloud_with_model_normals(dev, tmp_path):
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

    def pipeline(m=None):
        return SimpleNamespace(model=model if m is None else m, datamanager=TrainRayDataManager(
            sa.PixelBatcher(data, torch.arange(n_cam, device=dev), seed=3), 512))

    # a box whose upper x face removes about a fifth of the points
    every = generate_point_cloud(pipeline(), num_points=700, remove_outliers=False, use_bounding_box=False)
    big = float(every.points.abs().max()) + 1.0
    kw = dict(num_points=700, remove_outliers=True, std_ratio=1.0, bounding_box_min=(-big, -big, -big),
              bounding_box_max=(float(every.points[:, 0].quantile(0.8)), big, big))
    with pytest.raises(KeyError, match="normals"):
        generate_point_cloud(pipeline(), normal_method="model_output", **kw)      # the switch is off: no such output
    with pytest.raises(ValueError, match="0, 1"):
        generate_point_cloud(pipeline(_Shifted(model)), normal_method="model_output", **kw)
    plain = generate_point_cloud(pipeline(), **kw)
    model.config.render_normals = True
    pcd = generate_point_cloud(pipeline(), normal_method="model_output", estimate_normals=True, **kw)
    assert 0 < len(pcd) and torch.equal(pcd.points, plain.points) and torch.equal(pcd.colors, plain.colors)
    assert plain.normals is None
    assert pcd.normals.dtype == torch.float64 and pcd.normals.shape == pcd.points.shape
    norms = pcd.normals.norm(dim=1)
    assert bool(((norms - 1.0).abs() <= 1e-5).logical_or(norms == 0).all()) and float(norms.max()) > 0.5
    # without the filter: one normal per kept point, and fewer points survive the filter than enter it
    unfiltered = generate_point_cloud(pipeline(), normal_method="model_output", **dict(kw, remove_outliers=False))
    assert len(every) > len(unfiltered.normals) == len(unfiltered) > len(pcd)
    _, kept = unfiltered.remove_statistical_outlier(nb_neighbors=20, std_ratio=1.0)
    assert torch.equal(pcd.normals, unfiltered.normals[kept])
    out = export_point_cloud(pipeline(), tmp_path / "exports", normal_method="model_output", **kw)
    p, c, n = ply.read_point_cloud(str(tmp_path / "exports" / "point_cloud.ply"))
    assert np.array_equal(p, pcd.points.cpu().numpy()) and np.array_equal(n, pcd.normals.cpu().numpy())
    assert torch.equal(out.normals, pcd.normals)
    with open(tmp_path / "exports" / "point_cloud.ply", "rb") as fh:
        header = fh.read(400)
    assert b"property double nx" in header and b"property double ny" in header and b"property double nz" in header
