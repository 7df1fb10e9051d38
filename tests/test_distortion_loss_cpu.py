"""use_distortion_loss without a GPU: the float64 reference the GPU tests compare against checks itself, and the switch
exists through the layers — header, library export, ctypes binding, config."""
import os
import re

import pytest
import torch

from tests import distortion_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("S", [1, 2, 48, 130])
def test_reference_closed_form_gradient_is_its_own_autograd(S):
    """The closed-form dL/dw of tests/distortion_reference.py against float64 autograd of ns.lossfun_distortion, on the
    regime batch of tests/test_gpu_ray_kernels.py (empty, opaque, spike, zero-width bins, far, faint rays): 1e-12 of the
    ray's largest entry."""
    from tests.test_gpu_ray_kernels import _batch
    edges, dens, _, _ = _batch(S)
    spacing = dr.spacing_from_edges(edges)
    R = edges.shape[0]
    mult, up = 0.1, 0.37
    loss, w, gw, d_density = dr.reference(edges, spacing, dens, mult, up)
    closed = dr.closed_form_gw(spacing, w, mult * up / R)
    scale = gw.abs().max(1, keepdim=True).values
    assert float(scale.max()) > 0
    assert float(((closed - gw).abs() - 1e-12 * scale).max()) <= 0
    assert float(gw.min()) >= 0                       # every term of dD/dw is >= 0
    assert float(gw[0].abs().max()) == 0.0            # the empty ray
    assert torch.isfinite(d_density).all()
    assert abs(float(loss) - mult * up * float(dr.distortion_per_ray(spacing, w).mean())) <= 1e-15


def test_two_sample_closed_form():
    """S = 2: D = 2 a b |m1 - m2| + (a^2 d1 + b^2 d2) / 3."""
    t = torch.tensor([[0.1, 0.3, 0.9]], dtype=torch.float64)
    a, b = 0.25, 0.6
    w = torch.tensor([[a, b]], dtype=torch.float64)
    m1, m2, d1, d2 = 0.2, 0.6, 0.2, 0.6
    want = 2 * a * b * abs(m1 - m2) + (a * a * d1 + b * b * d2) / 3
    assert abs(float(dr.distortion_per_ray(t, w)) - want) <= 1e-15
    gw = dr.closed_form_gw(t, w, 1.0)
    assert abs(float(gw[0, 0]) - (2 * b * abs(m1 - m2) + 2 * a * d1 / 3)) <= 1e-15
    assert abs(float(gw[0, 1]) - (2 * a * abs(m1 - m2) + 2 * b * d2 / 3)) <= 1e-15


def test_header_declares_and_library_exports_the_backward():
    """include/fruitnerf_hip.h declares fnr_distortion_bwd, the built library exports it through the ctypes table, and
    the ABI is still 13 (a pure addition)."""
    from fruitnerf_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "fruitnerf_hip.h")).read()
    assert re.search(r"\bint\s+fnr_distortion_bwd\s*\(", header)
    assert "fnr_distortion_bwd" in L.SIGNATURES and len(L.SIGNATURES["fnr_distortion_bwd"][1]) == 12
    lib = L.load()
    assert hasattr(lib, "fnr_distortion_bwd")
    assert lib.fnr_abi_version() == 13 == L.ABI_VERSION
    # argument checks come before any launch (no device needed): S out of range, a null required pointer
    import ctypes as C
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.fnr_distortion_bwd(1, 0, p, p, p, p, 0.1, None, 0, None, p, None) != 0
    assert lib.fnr_distortion_bwd(1, 513, p, p, p, p, 0.1, None, 0, None, p, None) != 0
    assert lib.fnr_distortion_bwd(1, 4, p, p, p, p, 0.1, None, 0, None, None, None) != 0
    assert lib.fnr_distortion_bwd(0, 4, p, p, p, p, 0.1, None, 0, None, p, None) == 0      # no rays: nothing to launch


def test_config_default_is_off():
    from fruitnerf_amd.fruit_nerf import FruitNerfModelConfig
    cfg = FruitNerfModelConfig()
    assert cfg.use_distortion_loss is False
    assert cfg.distortion_loss_mult == 0.002
    from fruitnerf_amd import _kernels as K
    assert callable(K.distortion_bwd)
