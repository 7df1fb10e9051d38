"""float64 reference of use_distortion_loss (nerfstudio 0.3.2 distortion_loss on the final level), computed from float32
inputs: oracle/ns_torch.py's lossfun_distortion and RaySamples.get_weights in float64, differentiated by autograd.

    loss = mult * up * mean_r D_r,   D_r = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 ds_i

The spacing bins are constants (ns_torch.py: ray_samples_to_sdist works on detached bins), so the only gradient is
dL/dw_k = (mult * up / R) (2 sum_j w_j |m_k - m_j| + (2/3) w_k ds_k) — `closed_form_gw`, checked against autograd by
tests/test_distortion_loss_cpu.py — carried into the density by get_weights."""
import torch

from oracle import ns_torch as ns

F8 = torch.float64


def spacing_from_edges(edges: torch.Tensor) -> torch.Tensor:
    """Euclidean bin edges [R,S+1] -> spacing edges in [0, 1], in float32 (what the kernel is given)."""
    e = edges.float()
    span = e[:, -1:] - e[:, :1]
    return ((e - e[:, :1]) / torch.where(span > 0, span, torch.ones_like(span))).contiguous()   # (a ray of zero length: all 0)


def samples64(edges: torch.Tensor) -> ns.RaySamples:
    e = edges.double()
    return ns.RaySamples(frustums=ns.Frustums(None, None, e[:, :-1, None], e[:, 1:, None], None),
                         deltas=(e[:, 1:] - e[:, :-1])[..., None])


def distortion_per_ray(spacing: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """D_r [R] in float64 (ns.lossfun_distortion)."""
    return ns.lossfun_distortion(spacing.double(), w.double())


def closed_form_gw(spacing: torch.Tensor, w: torch.Tensor, coef: float) -> torch.Tensor:
    """coef * (2 sum_j w_j |m_k - m_j| + (2/3) w_k ds_k) [R,S], float64; coef = mult * up / R."""
    t, w = spacing.double(), w.double()
    m = (t[:, 1:] + t[:, :-1]) / 2
    ds = t[:, 1:] - t[:, :-1]
    inner = (w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum(-1)
    return coef * (2 * inner + 2 * w * ds / 3)


def reference(edges: torch.Tensor, spacing: torch.Tensor, density: torch.Tensor, mult: float, up: float = 1.0):
    """float64 autograd of mult * up * mean_r D_r through get_weights on the Euclidean `edges`.
    -> loss (scalar), weights [R,S], dL/dweights [R,S], dL/ddensity [R,S]."""
    s = density.double().clone().requires_grad_(True)
    w = samples64(edges).get_weights(s[..., None])[..., 0]
    w.retain_grad()
    loss = mult * up * distortion_per_ray(spacing, w).mean()
    loss.backward()
    return loss.detach(), w.detach(), w.grad.detach(), s.grad.detach()
