"""Analytic normals without a GPU: the formula fnr_field_normals evaluates against float64 autograd through the oracle's
FruitField, the float32 emulation of the kernel against the error bound the GPU tests use (and the constant of that bound),
the excluded samples and their cap, and the host-side checks of the new entry points, the config switch and the exporter."""
import copy
import ctypes as C

import pytest
import torch

from oracle import ns_torch as ns
from tests import normals_reference as nr
from tests import util


def _samples(R, S, seed, far):
    """Ray samples [R,S] in float64 around the scene, the last ray's samples at distance `far` (outside every box)."""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(R, 3, generator=g, dtype=torch.float64) - 0.5) * 1.2
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g, dtype=torch.float64), dim=-1)
    t = torch.rand(R, S + 1, generator=g, dtype=torch.float64).cumsum(1) * 0.08
    t[R - 1] = far
    rb = ns.RayBundle(o, d, torch.full((R, 1), 1e-6, dtype=torch.float64))
    return rb.get_ray_samples(bin_starts=t[:, :-1, None], bin_ends=t[:, 1:, None])


@pytest.mark.parametrize("contract", [True, False], ids=["contraction", "aabb"])
def test_formula_equals_float64_autograd_through_the_oracle_field(contract):
    cfg = util.small_config()
    cfg.disable_scene_contraction = not contract
    field = copy.deepcopy(util.make_oracle(cfg).field).double()
    R, S = 12, 16
    # contraction: 2 - 1 / 1e30 rounds to 2, (2 + 2) / 4 = 1 is not < 1; aabb: far outside the box
    rs = _samples(R, S, 3, far=1e30)
    field.get_density(rs)
    x = field._sample_locations
    assert x.dtype == torch.float64 and x.requires_grad
    gref = torch.autograd.grad(field._density_before_activation.sum(), x)[0].reshape(-1, 3)
    nref = -torch.nn.functional.normalize(gref, dim=-1)
    xs = x.detach().reshape(-1, 3)
    sel = ((xs > 0) & (xs < 1)).all(1)
    assert int((~sel).sum()) >= S and int(sel.sum()) >= 4 * S
    J, feats = nr.grid_jacobian(field.mlp_base_grid, xs)
    b = field.mlp_base_mlp.layers
    with torch.no_grad():
        g, _, _, _ = nr.formula(b[0].weight, b[0].bias, b[1].weight[0], feats, J)
        g = g * sel[:, None]
        normals = -g / g.norm(dim=1).clamp_min(1e-12)[:, None]
    scale = gref.abs().max()
    assert float((g - gref).abs().max()) <= 1e-12 * float(scale)
    assert float((normals - nref).abs().max()) <= 1e-10
    assert bool((gref[~sel] == 0).all()) and bool((normals[~sel] == 0).all()) and bool((nref[~sel] == 0).all())
    # the same through the helper the GPU test uses
    n2, g2 = nr.autograd_normals(field, xs)
    assert float((n2 - nref).abs().max()) <= 1e-12 and float((g2 - gref).abs().max()) <= 1e-12 * float(scale)


@pytest.mark.parametrize("shape", nr.SHAPE_LIST)
def test_float32_emulation_within_the_bound_and_the_constant(shape):
    """Every kept sample of the float32 emulation within C_NORMALS (2 E / ||g|| + 4 u); C_NORMALS >= 4 x the worst ratio; the
    excluded samples under 1 % of N — and with these fixtures none at all."""
    worst, worst_err, worst_cond = 0.0, 0.0, 0.0
    for R, S in nr.CASES:
        net, batch, jac = nr.case_inputs(shape, R, S)
        ref = nr.reference(net, batch, jac)
        kink = nr.kink_of_a1(net, batch, ref["f"])
        N = batch["N"]
        assert int(kink.sum()) < 0.01 * N, (shape, R, S, int(kink.sum()))
        assert int(kink.sum()) == 0, (shape, R, S)
        keep = ~kink
        n32, g32 = nr.emulate(net, batch, jac)
        unsel = ~batch["sel"]
        assert bool((n32[unsel] == 0).all()) and bool((g32[unsel] == 0).all()) and bool((ref["normals"][unsel] == 0).all())
        r = nr.ratios(n32, ref, keep)
        err = float((n32.double() - ref["normals"]).norm(dim=1)[keep].max())
        cond = float((ref["scale"].sum(1) / ref["norm"].clamp_min(1e-300))[keep & batch["sel"]].max())
        print(f"[normals cpu] {shape} ({R},{S}): worst ratio {float(r.max()):.3g}  |err| {err:.3g}  sum|df||J|/|g| {cond:.3g}")
        worst, worst_err, worst_cond = max(worst, float(r.max())), max(worst_err, err), max(worst_cond, cond)
        assert float(r.max()) <= nr.C_NORMALS
    print(f"[normals cpu] {shape}: worst ratio {worst:.3g} (C_NORMALS {nr.C_NORMALS}), |err| {worst_err:.3g}, cond {worst_cond:.3g}")
    assert 4.0 * worst <= nr.C_NORMALS


@pytest.mark.parametrize("shape", nr.SHAPE_LIST)
def test_the_bound_has_teeth_on_the_emulation(shape):
    """The wrong density row and two exchanged Jacobian axes miss the bound on every case, in the emulation already."""
    for R, S in nr.CASES:
        net, batch, jac = nr.case_inputs(shape, R, S)
        n32, _ = nr.emulate(net, batch, jac)
        keep = torch.ones(batch["N"], dtype=torch.bool)
        for kw in (dict(row=1), dict(swap_axes=(0, 2))):
            wrong = nr.reference(net, batch, jac, **kw)
            assert float(nr.ratios(n32, wrong, keep).max()) > nr.C_NORMALS, (shape, R, S, kw)


def test_render_reference_zero_weights():
    w = torch.zeros(2, 5)
    w[1] = torch.rand(5)
    n = torch.nn.functional.normalize(torch.randn(2, 5, 3), dim=-1)
    assert bool((nr.render_reference(w, n, False)[0] == 0).all()) and bool((nr.render_reference(w, n, True)[0] == 0.5).all())
    assert abs(float(nr.render_reference(w, n, False)[1].norm()) - 1.0) < 1e-9


# ---- host checks ------------------------------------------------------------------------------------------------------

def test_config_default_and_head_name():
    from fruitnerf_amd.fruit_field import FieldHeadNames
    from fruitnerf_amd.fruit_nerf import FruitNerfModelConfig
    assert FruitNerfModelConfig().render_normals is False
    assert FieldHeadNames.NORMALS.value == "normals"


def test_exporter_argument_validation():
    from fruitnerf_amd.export.exporter_utils import generate_point_cloud
    with pytest.raises(ValueError, match="normal_method"):
        generate_point_cloud(None, normal_method="predicted")
    import inspect
    p = inspect.signature(generate_point_cloud).parameters
    assert p["normal_method"].default == "open3d" and p["normal_output_name"].default == "normals"


def test_select_by_index_carries_normals():
    from fruitnerf_amd.clustering.clustering_base import PointCloud
    pts = torch.arange(15, dtype=torch.float64).view(5, 3)
    pcd = PointCloud(pts, pts / 20.0, "cpu")
    pcd.normals = -pts
    idx = torch.tensor([4, 0, 2])
    sub = pcd.select_by_index(idx)
    assert torch.equal(sub.points, pts[idx]) and torch.equal(sub.normals, -pts[idx]) and sub.normals.dtype == torch.float64
    assert PointCloud(pts, None, "cpu").select_by_index(idx).normals is None


def test_the_three_symbols_exist_and_reject_null_arguments():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    for name in ("fnr_field_normals", "fnr_render_normals", "fnr_depth_points_normals"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.fnr_abi_version() == 13
    net = L.fnr_field_net()
    assert lib.fnr_field_normals(None, 4, 1, 1, 1, 1, None, None) == -1 and b"field_normals" in lib.fnr_last_error()
    assert lib.fnr_field_normals(C.byref(net), 4, 1, 1, 1, None, None, None) == -1            # normals is required
    assert lib.fnr_field_normals(C.byref(net), 4, None, 1, 1, 1, None, None) == -1
    net.grid.n_levels, net.hidden_dim, net.geo_feat_dim = 16, 64, 20                           # a shape that is not built
    assert lib.fnr_field_normals(C.byref(net), 4, 1, 1, 1, 1, None, None) == -2
    net.geo_feat_dim = 15
    assert lib.fnr_field_normals(C.byref(net), 4, 1, 1, 1, 1, None, None) == -1 and b"weight" in lib.fnr_last_error()
    assert lib.fnr_render_normals(4, 8, None, 1, 0, 1, None) == -1 and b"render_normals" in lib.fnr_last_error()
    assert lib.fnr_render_normals(4, 8, 1, 1, 0, None, None) == -1
    assert lib.fnr_render_normals(4, 0, 1, 1, 0, 1, None) == -1                                # S out of range
    assert lib.fnr_depth_points_normals(1, 1, 1, 1, None, 4, None, None, 1, 1, 1, 4, 1, 1, None) == -1
    assert b"depth_points_normals" in lib.fnr_last_error()
    assert lib.fnr_depth_points_normals(1, 1, 1, 1, 1, 4, None, None, 1, 1, None, 4, 1, 1, None) == -1
    assert lib.fnr_depth_points_normals(None, 1, 1, 1, 1, 4, None, None, 1, 1, 1, 4, 1, 1, None) == -1
