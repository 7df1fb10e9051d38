"""Float64 references for background_color / use_gradient_scaling in the compositing kernels, written from the recalled
nerfstudio 0.3.2 definitions and from the published Philox4x32-10 (Salmon et al. 2011): shared by
tests/test_composite_background_cpu.py (which pins them on oracle/ns_torch.py and on the Random123 known-answer vector) and
tests/test_gpu_composite_background.py (which holds the kernels to them).

  out_rgb = sum_k w_k c_k + b (1 - sum_k w_k),  b = c_{S-1} ("last_sample": attached, it carries gradient) or an explicit
  constant triple; outside training the sample colours go through nan_to_num first and out_rgb is clamped to [0, 1] after.
  Gradient scaling: d_density_k, d_rgb_k, d_logit_k times s_k = clamp(((e_k + e_{k+1}) / 2)^2, 0, 1); forward unchanged.
"""
import numpy as np
import torch
import torch.nn.functional as F

F8 = torch.float64


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
RANDOM_BACKGROUND_GROUP = 2     # word groups 0 and 1 of a (seed, offset) belong to fnr_train_prologue


def philox4x32_10(counter: np.ndarray, key) -> np.ndarray:
    """counter [..., 4] uint32, key (k0, k1) -> [..., 4] uint32: ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by the Weyl
    constants after every round."""
    c = [counter[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & mask
        hi1, lo1 = p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def step_randoms(seed: int, offset: int, n_rays: int, group: int) -> np.ndarray:
    """The four numbers of word group `group` for rays 0 .. n_rays-1 of step `offset`: counter = (ray low word,
    ray high word ^ group << 24, offset low, offset high), key = the seed's two words, x -> (x >> 8) 2^-24 in [0, 1)."""
    r = np.arange(n_rays, dtype=np.uint64)
    counter = np.stack([r & np.uint64(0xFFFFFFFF), (r >> np.uint64(32)) ^ np.uint64((group << 24) & 0xFFFFFFFF),
                        np.full(n_rays, offset & 0xFFFFFFFF, np.uint64), np.full(n_rays, (offset >> 32) & 0xFFFFFFFF, np.uint64)],
                       -1).astype(np.uint32)
    words = philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return ((words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def random_background(seed: int, offset: int, n_rays: int) -> torch.Tensor:
    """What fnr_random_background writes: words 0-2 of group 2, [n_rays, 3] float32."""
    return torch.from_numpy(step_randoms(seed, offset, n_rays, RANDOM_BACKGROUND_GROUP)[:, :3].copy())


# ---- compositing ---------------------------------------------------------------------------------------------------
def weights64(edges: torch.Tensor, density: torch.Tensor) -> torch.Tensor:
    """RaySamples.get_weights in float64: [R,S] (density may require grad)."""
    e = edges.double()
    delta = e[:, 1:] - e[:, :-1]
    dd = delta * density
    excl = torch.cat([torch.zeros_like(dd[:, :1]), torch.cumsum(dd[:, :-1], 1)], 1)
    return torch.nan_to_num((1 - torch.exp(-dd)) * torch.exp(-excl))


def composite(w: torch.Tensor, rgb: torch.Tensor, background, training: bool) -> torch.Tensor:
    """RGBRenderer.combine_rgb: w [R,S], rgb [R,S,3] float64; background None (the last sample's colour, attached) or a
    [3] / [R,3] constant."""
    if not training:
        rgb = torch.nan_to_num(rgb)
    comp = (w[..., None] * rgb).sum(1)
    acc = w.sum(1)
    b = rgb[:, -1, :] if background is None else background.double().expand(rgb.shape[0], 3)
    out = comp + b * (1.0 - acc[:, None])
    return out if training else out.clamp(0.0, 1.0)


def distance_scale64(edges: torch.Tensor) -> torch.Tensor:
    m = (edges[:, :-1].double() + edges[:, 1:].double()) / 2
    return (m * m).clamp(0.0, 1.0)


def distance_scale32(edges: torch.Tensor) -> torch.Tensor:
    """s_k as the kernels form it: float32 add, halve, square, clamp."""
    e = edges.float()
    m = (e[:, :-1] + e[:, 1:]) / 2
    return (m * m).clamp(0.0, 1.0)


def backward(edges, density, rgb, logit, background=None, g_rgb=None, g_sem=None, image=None, mask=None,
             semantic_gradients=False, gradient_scaling=False, sem_weight=1.0):
    """float64 autograd of the training-mode composite under given per-ray gradients (g_rgb [R,3], g_sem [R]) or under
    MSE(out, image) + sem_weight BCEWithLogits(sem, mask).  -> dict: d_density [R,S], d_rgb [R,S,3], d_logit [R,S] (scaled by
    s_k with gradient_scaling), w, out, sem, g_rgb, g_sem (float64, what the loss put on the ray)."""
    s = density.double().clone().requires_grad_(True)
    c = rgb.double().clone().requires_grad_(True)
    lg = logit.double().clone().requires_grad_(True)
    w = weights64(edges, s)
    out = composite(w, c, background, True)
    sem = ((w if semantic_gradients else w.detach()) * lg).sum(1)
    if image is None:
        g_rgb, g_sem = g_rgb.double(), g_sem.double()
        loss = (out * g_rgb).sum() + (sem * g_sem).sum()
    else:
        loss = F.mse_loss(out, image.double()) + sem_weight * F.binary_cross_entropy_with_logits(sem, mask.double())
        g_rgb = 2 * (out - image.double()).detach() / out.numel()
        g_sem = sem_weight * (torch.sigmoid(sem) - mask.double()).detach() / sem.numel()
    loss.backward()
    d_density, d_rgb, d_logit = s.grad, c.grad, lg.grad
    if gradient_scaling:
        sc = distance_scale64(edges)
        d_density, d_rgb, d_logit = d_density * sc, d_rgb * sc[..., None], d_logit * sc
    return {"d_density": d_density, "d_rgb": d_rgb, "d_logit": d_logit, "w": w.detach(), "out": out.detach(),
            "sem": sem.detach(), "g_rgb": g_rgb, "g_sem": g_sem}
