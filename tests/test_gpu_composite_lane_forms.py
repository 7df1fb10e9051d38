"""The compositing kernels per samples-per-lane: fnr_composite_fwd_bwd_targets is fnr_composite_fwd (training) followed by
fnr_composite_bwd_targets, bit for bit, in the one-wide form (S = 7 and 48: the final level of a training step) and across the
boundary to the two-wide one (S = 65), without and with fnr_composite_options; R = 5 leaves three waves of the second
workgroup without a ray.  The rays are the first five of tests/test_gpu_ray_kernels.py's batch: empty, opaque at the first / last sample, a surface spike, zero-width bins —
suffix sums that are exactly zero, where the sign of a zero could show."""
import pytest
import torch

from tests import test_gpu_ray_kernels as rk

pytestmark = pytest.mark.gpu

R = 5


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("semgrad", [False, True])
@pytest.mark.parametrize("S", [7, 48, 65])
def test_fused_forward_backward_is_the_two_launches(dev, S, semgrad):
    K = rk._K()
    edges, dens, rgb, logit = (t[:R].contiguous().to(dev) for t in rk._batch(S, seed=11))
    g = torch.Generator().manual_seed(S)
    image = torch.rand(R, 3, generator=g).to(dev)
    mask = (torch.rand(R, generator=g) > 0.5).float().to(dev)
    rays = rk._rays(R, dev)
    rgb_n, logit_n = rgb.view(R * S, 3), logit.view(R * S)
    fwd = K.composite_fwd(rays, S, edges, dens, rgb_n, logit_n, True)
    weights, out_rgb, _, _, out_sem, _ = fwd
    if semgrad:
        bwd = K.composite_bwd_targets_semgrad(rays, S, edges, dens, rgb_n, logit_n, weights, out_rgb, image, out_sem, mask,
                                              rk.SEM_W)
    else:
        bwd = K.composite_bwd_targets(rays, S, edges, dens, rgb_n, weights, out_rgb, image, out_sem, mask, rk.SEM_W)
    fwd2, bwd2 = K.composite_fwd_bwd_targets(rays, S, edges, dens, rgb_n, logit_n, image, mask, rk.SEM_W, semgrad=semgrad)
    names = ("weights", "rgb", "accumulation", "depth", "semantics", "label", "d_density", "d_rgb", "d_logit")
    for name, a, b in zip(names, tuple(fwd) + tuple(bwd), tuple(fwd2) + tuple(bwd2)):
        assert torch.equal(a, b), name
        assert torch.equal(_bits(a), _bits(b)), f"{name}: a zero changed sign"   # (== takes -0.0 for +0.0)
    assert float(bwd[0].abs().max()) > 0


@pytest.mark.parametrize("options", ["white+scaling", "per_ray_background+semgrad", "last_sample+scaling+semgrad"])
@pytest.mark.parametrize("S", [7, 48, 65])
def test_fused_forward_backward_under_options_is_the_two_launches(dev, S, options):
    """The same under fnr_composite_options, whose kernels take the narrowest lane form like the plain ones:
    composite_fwd_bwd_targets_opt is composite_fwd_opt followed by composite_bwd_targets_opt, bit for bit."""
    K = rk._K()
    edges, dens, rgb, logit = (t[:R].contiguous().to(dev) for t in rk._batch(S, seed=11))
    g = torch.Generator().manual_seed(S)
    image = torch.rand(R, 3, generator=g).to(dev)
    mask = (torch.rand(R, generator=g) > 0.5).float().to(dev)
    background = {"white": torch.ones(3), "per_ray_background": torch.rand(R, 3, generator=g), "last_sample": None}[
        options.split("+")[0]]
    opts = K.CompositeOptions(None if background is None else background.to(dev), "scaling" in options, "semgrad" in options)
    rays = rk._rays(R, dev)
    rgb_n, logit_n = rgb.view(R * S, 3), logit.view(R * S)
    fwd = K.composite_fwd_opt(rays, S, edges, dens, rgb_n, logit_n, True, opts)
    weights, out_rgb, _, _, out_sem, _ = fwd
    bwd = K.composite_bwd_targets_opt(rays, S, edges, dens, rgb_n, logit_n, weights, out_rgb, image, out_sem, mask, rk.SEM_W,
                                      opts)
    fwd2, bwd2 = K.composite_fwd_bwd_targets_opt(rays, S, edges, dens, rgb_n, logit_n, image, mask, rk.SEM_W, opts)
    names = ("weights", "rgb", "accumulation", "depth", "semantics", "label", "d_density", "d_rgb", "d_logit")
    for name, a, b in zip(names, tuple(fwd) + tuple(bwd), tuple(fwd2) + tuple(bwd2)):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: differs, or a zero changed sign"   # (== takes -0.0 for +0.0)
    assert float(bwd[0].abs().max()) > 0
