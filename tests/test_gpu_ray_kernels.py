"""Per-ray kernels (one 64-lane wave per ray, sample k in lane k / E, element k % E, E = ceil(S / 64) <= 8) against
oracle/ns_torch.py evaluated in float64, per element and per ray — never against a batch maximum.

Every batch puts each regime in its own ray next to ordinary random rays (R = 15: not a multiple of the 4 rays of a
workgroup): an empty ray, rays opaque at the first / last sample, a surface spike, zero-width bins, a ray out to
t = 1000, a faint ray (densities 1e-3 of the others), rays whose first weight is exactly 1/2 (the median's `>=`), and
composited logits beyond +-17.  The kernels that chunk a ray over the lanes (compositing forward and backward, the
weights backward, k_weights_pdf, the interlevel scans of the proposal level, alone and inside k_train_losses) run at
every E from 1 to 8 with full and partial last lanes; the distortion and ray-gradient kernels stride a ray over the lanes.

Bounds (measured worst value / bound, on an MI355X, in brackets).  Besides the ceilings (2e-6 relative for forward
quantities, 1e-5 per ray for gradients, 1e-4 of the two-term scale for d_density) some bounds carry a term that follows
from float32 arithmetic the float32 reference shares, stated where it is used:
  * A_k = T_k (4u + (E + 7) u X_k), u = 2^-24, X_k = sum_{j<k} delta_j sigma_j, T_k = exp(-X_k): the absolute error of a
    float32 weight.  `1 - exp(-delta sigma)` is rounded in absolute terms (4u) and the exclusive scan that forms X_k has
    depth E + 6, so T_k carries a relative error <= (E + 7) u X_k.
  * |sigma(x) - y| for y = 1, x > 16.6 (and y = 0, x < -16.6) is 0 in float32 and ~e^-|x| exactly: d_sem / d_logit carry an
    absolute term w 2^-22 / R.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ns_torch as ns

pytestmark = pytest.mark.gpu

F8 = torch.float64
U = 2.0 ** -24
# every E = ceil(S / 64) from 1 to 8, each with a full last lane (S % E == 0) and, for E >= 2, a partial one
SS = (1, 2, 48, 64, 65, 96, 129, 130, 200, 255, 256, 320, 321, 383, 384, 447, 448, 511, 512)
SEM_W = 1.0
R_REG = 15          # rays per batch: 9 regime rays + 6 random, R % 4 == 3


def _K():
    from fruitnerf_amd import _kernels as K
    return K


def _worst(name, ratio):
    v = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[ray kernels] {name}: worst |err| / bound = {v:.3g}")
    return v


# ---------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------

def _batch(S, seed=0):
    """edges [R,S+1], density [R,S], rgb [R,S,3], logit [R,S] (float32, CPU).  Rows 0-8 are the regimes."""
    g = torch.Generator().manual_seed(7919 * S + seed)
    R = R_REG
    steps = torch.rand(R, S + 1, generator=g) * 0.05 + 0.01
    steps[4, 1::3] = 0.0                                              # zero-width bins (every third)
    edges = torch.cumsum(steps, 1)
    edges[5] = edges[5] / edges[5, -1] * 1000.0                       # t up to 1000
    edges[6:9] = torch.arange(S + 1, dtype=torch.float32)             # delta = 1 exactly
    dens = torch.rand(R, S, generator=g) * (3.0 / (S * 0.035))        # optical depth ~1.5 over a random ray
    dens[0] = 0.0                                                     # empty ray
    dens[1, 0] = 1e8                                                  # opaque at the first sample
    dens[2] = 0.0
    dens[2, -1] = 1e8                                                 # opaque at the last sample
    dens[3, S // 2] = 1e7                                             # surface spike
    dens[4, 1::3] = 1e9                                               # ... on the zero-width bins
    dens[5] *= 1e-3                                                   # faint ray (and far)
    ln2 = torch.tensor(math.log(2.0), dtype=torch.float32)
    half = torch.stack([torch.nextafter(ln2, torch.tensor(0.0)), ln2, torch.nextafter(ln2, torch.tensor(1.0))])
    dens[6:9] = 0.5 * dens[6:9] / (3.0 / (S * 0.035))                 # small behind the first sample
    dens[6:9, 0] = half                                               # 1 - exp(-ln2) = 1/2: the median's ">=" decides
    rgb = torch.rand(R, S, 3, generator=g) * 1.4 - 0.2                # outside [0,1]: the eval clamp acts
    logit = torch.randn(R, S, generator=g) * 4.0
    logit[1] = 40.0                                                   # composited logit +40 (opaque ray)
    logit[2] = -40.0
    return edges.contiguous(), dens.contiguous(), rgb.contiguous(), logit.contiguous()


def _rays(R, dev, near=0.05, far=1000.0, o=None, d=None):
    K = _K()
    o = torch.zeros(R, 3) if o is None else o
    d = torch.tensor([[0.0, 0.0, 1.0]]).repeat(R, 1) if d is None else d
    return K.RaysArg(o.to(dev), d.to(dev), torch.full((R, 1), near, device=dev), torch.full((R, 1), far, device=dev))


def _samples64(edges):
    e = edges.double()
    return ns.RaySamples(frustums=ns.Frustums(None, None, e[:, :-1, None], e[:, 1:, None], None),
                         deltas=(e[:, 1:] - e[:, :-1])[..., None])


def _transmittance(edges, dens):
    """float64 X_k (exclusive optical depth), T_k, T_{k+1}."""
    dd = (edges[:, 1:] - edges[:, :-1]).double() * dens.double()
    incl = torch.cumsum(dd, 1)
    X = torch.cat([torch.zeros_like(dd[:, :1]), incl[:, :-1]], 1)
    return X, torch.exp(-X), torch.exp(-incl)


def _weight_arith(edges, dens):
    S = dens.shape[1]
    E = (S + 63) // 64
    X, T, _ = _transmittance(edges, dens)
    return T * (4 * U + (E + 7) * U * X)


def _check_median(name, depth, edges, w64):
    """The kernel's median index (recovered from its depth: the float32 midpoint (e_k + e_k+1) / 2 is the kernel's own
    arithmetic) must equal the float64 one, except where the float64 cumulative weight at the deciding sample is within
    1e-6 of 0.5."""
    S = w64.shape[1]
    mids = (edges[:, :-1] + edges[:, 1:]) / 2
    cw = torch.cumsum(w64, 1)
    for r in range(w64.shape[0]):
        ref = min(int(torch.searchsorted(cw[r], torch.tensor([0.5], dtype=F8), side="left")), S - 1)
        allowed = {ref}
        near = (cw[r] - 0.5).abs() <= 1e-6
        for j in torch.nonzero(near).flatten().tolist():
            allowed |= {j, min(j + 1, S - 1)}
        got = set(torch.nonzero(mids[r] == depth[r]).flatten().tolist())
        assert got & allowed, f"{name}: ray {r} median index {sorted(got)} not in {sorted(allowed)}"


# ---------------------------------------------------------------------------------------------------------------------
# compositing forward
# ---------------------------------------------------------------------------------------------------------------------

def _composite_ref(edges, dens, rgb, logit, training):
    rs = _samples64(edges)
    w = rs.get_weights(dens.double()[..., None])
    c = ns.render_rgb_last_sample(rgb.double(), w, training)
    acc = ns.render_accumulation(w)[:, 0]
    sem = ns.render_semantics(logit.double()[..., None], w)[:, 0]
    return w[..., 0], c, acc, sem


@pytest.mark.parametrize("training", [True, False])
def test_composite_forward_per_ray(dev, training):
    """k_composite_fwd (training and eval: nan_to_num + clamp) at every S: weights, rgb (last-sample background),
    accumulation, median depth, semantics and label.  [w 0.15, rgb 0.04, acc 0.031, sem 0.035]"""
    K = _K()
    worst = {}
    for S in SS:
        edges, dens, rgb, logit = _batch(S)
        if not training:
            rgb[3, S // 2 + 1:, 1] = float("nan")                       # behind the spike: nan_to_num in eval only
        R = edges.shape[0]
        w, out, acc, depth, sem, label = K.composite_fwd(_rays(R, dev), S, edges.to(dev), dens.to(dev), rgb.to(dev),
                                                         logit.to(dev), training)
        w, out, acc, depth, sem, label = (t.cpu() for t in (w, out, acc, depth, sem, label))
        w64, c64, acc64, sem64 = _composite_ref(edges, dens, rgb, logit, training)
        A = _weight_arith(edges, dens)
        wmax = w64.max(1, keepdim=True).values
        worst.setdefault("w", []).append(((w.double() - w64).abs() / (2e-6 * wmax + A + 1e-300)).max())
        ca = torch.nan_to_num(rgb.double()).abs()
        s_rgb = 2e-6 * ((w64[..., None] * ca).sum(1) + ca[:, -1] * (1 + acc64[:, None])) + \
            (A[..., None] * (ca + ca[:, -1:])).sum(1)
        worst.setdefault("rgb", []).append(((out.double() - c64).abs() / s_rgb).max())
        worst.setdefault("acc", []).append(((acc.double() - acc64).abs() / (2e-6 * acc64 + A.sum(1) + 1e-300)).max())
        la = logit.double().abs()
        s_sem = 2e-6 * (w64 * la).sum(1) + (A * la).sum(1)
        worst.setdefault("sem", []).append(((sem.double() - sem64).abs() / (s_sem + 1e-300)).max())
        _check_median(f"composite S={S}", depth, edges, w64)
        sig = torch.sigmoid(sem64)
        decided = (sig - 0.9).abs() > 1e-5
        assert torch.equal(label[decided], (sig[decided] > 0.9).long()), f"label S={S}"
        # the exact half: first weight 1/2 -> median at sample 0 (when the device's expf returns exactly 1/2)
        exact = [r for r in (6, 7, 8) if float(w[r, 0]) == 0.5]
        for r in exact:
            assert float(depth[r]) == float((edges[r, 0] + edges[r, 1]) / 2), f"S={S} ray {r}: median at an exact 1/2"
        assert exact or S == 1, "no ray has a first weight of exactly 1/2"
        assert float(sem64[1]) > 17 and float(sem64[2]) < -17
    for k, v in worst.items():
        assert _worst(f"composite_fwd[{'train' if training else 'eval'}].{k}", torch.stack(v)) <= 1.0, k


# ---------------------------------------------------------------------------------------------------------------------
# compositing backward and the weights backward
# ---------------------------------------------------------------------------------------------------------------------

def _suffix(x):
    return torch.flip(torch.cumsum(torch.flip(x, [1]), 1), [1]) - x


def _two_term_scale(edges, dens, w64, gw_abs, gw_err=None):
    """-> 1e-4 delta_k (|gw_k| T_{k+1} + sum_{j>k} |gw_j| w_j) (the magnitude of the two terms d_density subtracts) plus the
    float32 underflow floor delta_k (|gw_k| + sum_{j>k} |gw_j|) 2^-126: where T < 2^-126 (optical depth > 87, reached on the
    long unit-step rays at S >= 448) the kernel's exp(-x) and the weights behind it are 0 or subnormal.  gw_err: an absolute
    error of the upstream gradient itself, carried through the same two terms at full weight."""
    _, _, Tn = _transmittance(edges, dens)
    delta = (edges[:, 1:] - edges[:, :-1]).double()
    scale = delta * (gw_abs * Tn + _suffix(gw_abs * w64))
    floor = delta * (gw_abs + _suffix(gw_abs)) * 2.0 ** -126
    if gw_err is not None:
        floor = floor + delta * (gw_err * Tn + _suffix(gw_err * w64))
    return 1e-4 * scale + floor, delta


def _composite_bwd_ref(edges, dens, rgb, logit, g_rgb=None, g_sem=None, image=None, mask=None):
    s = dens.double().requires_grad_(True)
    c = rgb.double().requires_grad_(True)
    lg = logit.double().requires_grad_(True)
    w = _samples64(edges).get_weights(s[..., None])
    out = ns.render_rgb_last_sample(c, w, True)
    sem = ns.render_semantics(lg[..., None], w.detach())[:, 0]           # semantic weights are detached
    if image is None:
        loss = (out * g_rgb.double()).sum() + (sem * g_sem.double()).sum()
    else:
        loss = F.mse_loss(out, image.double()) + SEM_W * F.binary_cross_entropy_with_logits(sem, mask.double())
        g_rgb = 2 * (out - image.double()).detach() / out.numel()
        g_sem = SEM_W * (torch.sigmoid(sem) - mask.double()).detach() / sem.numel()
    loss.backward()
    gw_abs = (g_rgb.double().abs()[:, None, :] * (rgb.double() - rgb.double()[:, -1:, :]).abs()).sum(-1)
    return s.grad, c.grad, lg.grad, w.detach()[..., 0], gw_abs, g_sem.double(), g_rgb.double().abs()


def _check_composite_grads(name, worst, edges, dens, logit, sem64, got, ref, R, inputs):
    """inputs: "given" (composite_bwd: weights w64 rounded to float32, per-ray gradients given), "rounded"
    (composite_bwd_targets: also the composite and the composited logit rounded to float32) or "own" (the fused launch
    reads its own forward).  The rounded inputs carry u w_k and u |sem|; the fused launch's own forward carries A_k in the
    weights and the forward bound on the composited logit."""
    d_s, d_c, d_l = (t.cpu().double().view(R, -1, *t.shape[1:]) for t in got)
    r_s, r_c, r_l, w64, gw_abs, g_sem, g_rgb_abs = ref
    S = w64.shape[1]
    if inputs == "own":
        A = _weight_arith(edges, dens)
        la = logit.double().abs()
        sem_err = 2e-6 * (w64 * la).sum(1) + (A * la).sum(1)
    else:
        A = U * w64
        sem_err = U * sem64.abs() if inputs == "rounded" else torch.zeros_like(sem64)
    scale, _ = _two_term_scale(edges, dens, w64, gw_abs)
    worst.setdefault(f"{name}.d_density", []).append(((d_s.view_as(r_s) - r_s).abs() / (scale + 1e-300)).max())
    cmax = r_c.abs().flatten(1).max(1).values[:, None, None]
    # the background share 1 - sum_k w_k is a float32 difference: absolute error (E + 6) u + sum_k A_k (the input weights')
    bg_err = torch.zeros_like(r_c)
    bg_err[:, -1, :] = g_rgb_abs * ((S + 63) // 64 + 6) * U + g_rgb_abs * A.sum(1, keepdim=True)
    bnd = 1e-5 * cmax + bg_err + g_rgb_abs[:, None, :] * A[..., None]
    worst.setdefault(f"{name}.d_rgb", []).append(((d_c.view_as(r_c) - r_c).abs() / (bnd + 1e-300)).max())
    lmax = r_l.abs().max(1, keepdim=True).values
    floor = SEM_W * 2.0 ** -22 / R * w64
    # the targets launches form gs = w (sigmoid(sem) - mask) / R from the composited logit they read (error sem_err) and
    # multiply it by the weights they read (error A_k)
    sig = torch.sigmoid(sem64)
    d_gs = SEM_W / R * sig * (1 - sig) * sem_err
    bnd = 1e-5 * lmax + floor + g_sem.abs()[:, None] * A + d_gs[:, None] * (w64 + A)
    worst.setdefault(f"{name}.d_logit", []).append(((d_l.view_as(r_l) - r_l).abs() / (bnd + 1e-300)).max())


def test_composite_backward_per_element(dev):
    """composite_bwd (given per-ray gradients), composite_bwd_targets and composite_fwd_bwd_targets (MSE + w BCE formed in
    the kernel) against float64 autograd through get_weights + render_rgb_last_sample + render_semantics (semantic
    weights detached): d_density per element against the two-term scale (1e-4), d_rgb (incl. the k = S-1 background
    share) and d_logit per ray (1e-5).  The image is the float64 composite + 0.25 (the MSE gradient of an image that
    equals the composite is ill-conditioned in the composite's own rounding).  Every launch's background share
    1 - sum w is a float32 difference ((E + 6) u).  The separate launches read float64 results rounded to float32 (u w_k,
    u |sem|); only the fused launch's bounds add the error of its own forward: A_k in the weights and in the background
    share, and sigmoid'(sem) times the forward bound on the composited logit in the semantic gradient.
    [bwd: d_density 0.077, d_rgb 0.026, d_logit 0.009; targets: 0.078, 0.036, 0.083; fused: 0.15, 0.16, 0.14]"""
    K = _K()
    worst = {}
    for S in SS:
        edges, dens, rgb, logit = _batch(S)
        R = edges.shape[0]
        w64, c64, _, sem64 = _composite_ref(edges, dens, rgb, logit, True)
        g = torch.Generator().manual_seed(S)
        g_rgb = torch.randn(R, 3, generator=g)
        g_sem = torch.randn(R, generator=g)
        image = (c64 + 0.25).float()
        mask = (torch.arange(R) % 2).float()
        mask[1], mask[2] = 0.0, 1.0                                      # logits +-40 on the wrong side: |grad| ~ 1
        rays = _rays(R, dev)
        ev, dv, cv, lv = edges.to(dev), dens.to(dev), rgb.to(dev), logit.to(dev)
        wk = w64.float().to(dev)                                        # the backward on its own input
        got = K.composite_bwd(rays, S, ev, dv, cv, wk, g_rgb.to(dev), g_sem.to(dev))
        ref_g = _composite_bwd_ref(edges, dens, rgb, logit, g_rgb, g_sem)
        _check_composite_grads("composite_bwd", worst, edges, dens, logit, sem64, got, ref_g, R, "given")
        ref_t = _composite_bwd_ref(edges, dens, rgb, logit, image=image, mask=mask)
        got = K.composite_bwd_targets(rays, S, ev, dv, cv, wk, c64.float().to(dev), image.to(dev),
                                      sem64.float().to(dev), mask.to(dev), SEM_W)
        _check_composite_grads("composite_bwd_targets", worst, edges, dens, logit, sem64, got, ref_t, R, "rounded")
        _, got = K.composite_fwd_bwd_targets(rays, S, ev, dv, cv, lv, image.to(dev), mask.to(dev), SEM_W)
        # fused: the weights and the composited outputs are the kernel's own forward; their errors enter the bounds
        _check_composite_grads("composite_fwd_bwd_targets", worst, edges, dens, logit, sem64, got, ref_t, R, "own")
    for k, v in worst.items():
        assert _worst(k, torch.stack(v)) <= 1.0, k


def test_weights_bwd_with_upstream_every_layout(dev):
    """k_weights_bwd with a non-unit device `upstream` scalar at every E: d_density per element against float64 autograd
    of sum_k up g_k w_k, bounded by 1e-4 of the two-term scale.  [0.10]"""
    K = _K()
    ratios = []
    up = 0.37
    for S in SS:
        edges, dens, _, _ = _batch(S)
        R = edges.shape[0]
        g = torch.Generator().manual_seed(S + 11)
        gw = torch.randn(R, S, generator=g)
        gw[3] *= 1e-3                                                    # a ray whose gradient is far below the others
        s = dens.double().requires_grad_(True)
        w = _samples64(edges).get_weights(s[..., None])[..., 0]
        (w * gw.double() * up).sum().backward()
        got = K.weights_bwd(S, edges.to(dev), dens.to(dev), w.detach().float().to(dev), gw.to(dev),
                            torch.full((1,), up, device=dev)).cpu().double().view(R, S)
        scale, _ = _two_term_scale(edges, dens, w.detach(), (gw.double() * up).abs())
        ratios.append(((got - s.grad).abs() / (scale + 1e-300)).max())
    assert _worst("weights_bwd", torch.stack(ratios)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# weights + median + inverse-CDF resampling
# ---------------------------------------------------------------------------------------------------------------------

def _spacing_fns(kind):
    if kind == 0:
        return (lambda x: x), (lambda x: x)
    return (lambda x: torch.where(x < 1, x / 2, 1 - 1 / (2 * x))), (lambda x: torch.where(x < 0.5, 2 * x, 1 / (2 - 2 * x)))


def _inverse_cdf_slope(edges, wa, s):
    """ds/du of the inverse of the padded histogram CDF at s (the largest of the bin s falls in and its neighbours)."""
    pdf = wa + 0.01
    pdf = pdf / pdf.sum(1, keepdim=True)
    slope = (edges[:, 1:] - edges[:, :-1]).double() / pdf
    k = (torch.searchsorted(edges.double().contiguous(), s.contiguous(), side="right") - 1).clamp(0, pdf.shape[1] - 1)
    n = pdf.shape[1] - 1
    return torch.maximum(torch.gather(slope, 1, k), torch.maximum(torch.gather(slope, 1, (k - 1).clamp(min=0)),
                                                                  torch.gather(slope, 1, (k + 1).clamp(max=n))))


@pytest.mark.parametrize("S_prev", SS)
def test_weights_pdf_every_stage(dev, S_prev):
    """k_weights_pdf: weights, median depth, and the new spacing bins of PDFSampler (train with `rand`, eval without) at
    anneal 0 / 0.37 / 1, spacing kind 0 / 1, S_new 1 / 48 / 96 / 512, against float64 ProposalNetworkSampler pieces
    (torch.pow(w, anneal) then PDFSampler).  The euclidean bins are checked against the float64 transform of the
    kernel's OWN spacing bins and the spacing bins against PDFSampler fed the kernel's OWN weights, so each stage is
    checked on its own input (an anneal exponent a < 1 turns the float32 weights' absolute error into a relative error
    a dw / w of w^a, unbounded as w -> 0, in the histogram).  Kind 0: e = x s_far + (1 - x) s_near, a sum of two
    non-negative float32 products, is relatively accurate to a few u: |de| <= 2e-6 e.  Kind 1: |de| <= 2e-6 e + 2^-21 e^2 —
    s is formed in float32 (x s_far + (1 - x) s_near, |ds| <= 2^-22) and e = 1 / (2 - 2s) turns ds into de = 2 e^2 ds.
    Spacing bins (in [0, 1]): 2e-6 absolute plus (E + 8) u times the slope ds/du of the float64 inverse CDF at the bin — the
    CDF is a float32 scan of depth E + 6 over values <= 1 (|dcdf| <= (E + 8) u), and the inverse CDF multiplies that by
    width / mass of the bin (up to ~50 where a wide bin holds only the histogram padding at anneal 0.37).
    [w 0.16, spacing 0.28, euclid 0.34]"""
    K = _K()
    worst = {}
    near, far = 0.05, 1000.0
    edges, dens, _, _ = _batch(S_prev, seed=3)
    R = edges.shape[0]
    w64 = _samples64(edges).get_weights(dens.double()[..., None])[..., 0]
    A = _weight_arith(edges, dens)
    E = (S_prev + 63) // 64
    g = torch.Generator().manual_seed(S_prev)
    for kind in (0, 1):
        fn, inv = _spacing_fns(kind)
        # the kernel reads near / far as float32: the reference starts from the same values
        lo, hi = (float(fn(torch.tensor(v, dtype=torch.float32).double())) for v in (near, far))
        sp = torch.sort(torch.rand(R, S_prev + 1, generator=g), 1).values
        sp[:, 0], sp[:, -1] = 0.0, 1.0
        spacing_prev = sp.contiguous()

        def to_euclid(x):
            return inv(x * hi + (1 - x) * lo)
        rs_prev = ns.RaySamples(frustums=None, spacing_starts=spacing_prev.double()[:, :-1, None],
                                spacing_ends=spacing_prev.double()[:, 1:, None], spacing_to_euclidean_fn=to_euclid)
        rb = ns.RayBundle(torch.zeros(R, 3, dtype=F8), torch.zeros(R, 3, dtype=F8), torch.ones(R, 1, dtype=F8))
        for anneal in (0.0, 0.37, 1.0):
            for S_new in (1, 48, 96, 512):
                for training in (True, False):
                    rand = torch.rand(R, generator=g) if training else None
                    w, depth, sp_new, eu_new = K.weights_pdf(_rays(R, dev, near, far), kind, S_prev, S_new, dens.to(dev),
                                                             spacing_prev.to(dev), edges.to(dev), anneal,
                                                             None if rand is None else rand.to(dev))
                    w, depth, sp_new, eu_new = (t.cpu() for t in (w, depth, sp_new, eu_new))
                    wmax = w64.max(1, keepdim=True).values
                    worst.setdefault("w", []).append(((w.double() - w64).abs() / (2e-6 * wmax + A + 1e-300)).max())
                    _check_median(f"weights_pdf S_prev={S_prev}", depth, edges, w64)
                    exact = [r for r in (6, 7, 8) if float(w[r, 0]) == 0.5]
                    for r in exact:
                        assert float(depth[r]) == float((edges[r, 0] + edges[r, 1]) / 2), "median at an exact 1/2"
                    assert exact or S_prev == 1, "no ray has a first weight of exactly 1/2"
                    smp = ns.PDFSampler(num_samples=S_new, include_original=False, single_jitter=True)
                    smp.train(training)
                    wa = torch.pow(w.double(), anneal)      # the resampling stage on the kernel's own weights
                    out = smp(rb, rs_prev, wa[..., None], rand=None if rand is None else rand.double()[:, None])
                    ref_sp = torch.cat([out.spacing_starts[..., 0], out.spacing_ends[..., -1:, 0]], -1)
                    b = 2e-6 + _inverse_cdf_slope(spacing_prev, wa, ref_sp) * (E + 8) * U
                    worst.setdefault("spacing", []).append(((sp_new.double() - ref_sp).abs() / b).max())
                    e_ref = to_euclid(sp_new.double())
                    b = 2e-6 * e_ref.abs() + (2.0 ** -21 * e_ref ** 2 if kind == 1 else 0.0)
                    worst.setdefault("euclid", []).append(((eu_new.double() - e_ref).abs() / b).max())
                    assert torch.isfinite(sp_new).all()
    for k, v in worst.items():
        assert _worst(f"weights_pdf[{S_prev}].{k}", torch.stack(v)) <= 1.0, k


# ---------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------

def _dyadic_hist(R, S, g, ties_from=None):
    """Spacing edges (0 and 1 shared exactly, as in production) and weights on a 2^-12 grid: the float32 cumulative sums
    the interlevel loss differences are then exact, and the bounds measure the kernel's arithmetic, not the conditioning
    of w - w_outer."""
    t = torch.sort(torch.rand(R, S + 1, generator=g), 1).values
    t[:, 0], t[:, -1] = 0.0, 1.0
    if ties_from is not None:        # final edges taken from the proposal's interior edges: the side="right" rule
        Sp = ties_from.shape[1] - 1
        for r in range(0, R, 2):
            idx = torch.sort(torch.randint(1, max(Sp, 2), (S + 1,), generator=g)).values.clamp(max=Sp)
            t[r] = ties_from[r, idx]
            t[r, 0], t[r, -1] = 0.0, 1.0
            t[r] = torch.sort(t[r]).values
    w = torch.floor(torch.rand(R, S, generator=g) ** 3 * (8192.0 / S)) / 4096.0
    w[1] = 0.0                                                      # an empty ray
    return t.contiguous(), w.contiguous()


def _interlevel_ref(c, w, cp, wp, R, S_f, mult):
    wp64 = wp.double().requires_grad_(True)
    per = ns.lossfun_outer(c.double(), w.double(), cp.double(), wp64)          # [R, S_f]
    total = mult * per.mean()
    total.backward()
    return mult * per.sum(1) / (R * S_f), wp64.grad


@pytest.mark.parametrize("S_f,S_p", [(1, 1), (48, 64), (200, 65), (96, 96), (65, 129), (129, 130), (96, 255), (48, 256),
                                     (512, 320), (64, 321), (256, 383), (33, 384), (320, 447), (129, 448), (200, 511),
                                     (512, 512)])
def test_interlevel_per_ray_loss_and_gradient(dev, S_f, S_p):
    """k_interlevel: each ray's loss (R <= 128: every ray owns its accumulator slot) relative 2e-6, and d_wp per ray 1e-5,
    against float64 ns.lossfun_outer / autograd; half the rays take their final edges from the proposal's interior edges
    (ties: searchsorted side="right").  S_p covers every E_p = ceil(S_p / 64) with full and partial last lanes (the cy and
    d_wp scans are lane-chunked; the final level is strided over the lanes).  [loss 0.083, d_wp 0.034]"""
    K = _K()
    from fruitnerf_amd import _lib as L
    R, mult = 23, 1.0
    g = torch.Generator().manual_seed(S_f * 1000 + S_p)
    cp, wp = _dyadic_hist(R, S_p, g)
    c, w = _dyadic_hist(R, S_f, g, ties_from=cp)
    acc = torch.zeros(L.FNR_LOSS_SLOTS, device=dev)
    d_wp = K.interlevel_fwd(S_f, c.to(dev), w.to(dev), S_p, cp.to(dev), wp.to(dev), mult, acc).cpu().double()
    slots = acc.cpu().double()
    got = torch.stack([slots[(r // 4) * 32 + r % 4] for r in range(R)])
    ref, ref_g = _interlevel_ref(c, w, cp, wp, R, S_f, mult)
    assert float(ref.max()) > 0
    a = _worst(f"interlevel[{S_f},{S_p}].loss", (got - ref).abs() / (2e-6 * ref.abs() + 1e-30))
    gmax = ref_g.abs().max(1, keepdim=True).values
    b = _worst(f"interlevel[{S_f},{S_p}].d_wp", (d_wp - ref_g).abs() / (1e-5 * gmax + 1e-30))
    assert a <= 1.0 and b <= 1.0


@pytest.mark.parametrize("S", [1, 2, 65, 129, 256, 448, 512])
def test_distortion_per_ray(dev, S):
    """k_distortion per ray (R <= 128: one slot per ray) against float64 ns.lossfun_distortion (chunked over rays: the
    reference is O(R S^2)).  Every term is >= 0, so relative 2e-6.  [0.085]"""
    K = _K()
    from fruitnerf_amd import _lib as L
    R = 27
    g = torch.Generator().manual_seed(S)
    t, w = _dyadic_hist(R, S, g)
    w = w * (torch.rand(R, 1, generator=g) + 0.01)
    w = w.float().contiguous()
    out = torch.zeros(L.FNR_LOSS_SLOTS, device=dev)
    K.distortion(S, t.to(dev), w.to(dev), out=out)
    slots = out.cpu().double()
    got = torch.stack([slots[(r // 4) * 32 + r % 4] for r in range(R)])
    ref = torch.cat([ns.lossfun_distortion(t[a:a + 8].double(), w[a:a + 8].double()) for a in range(0, R, 8)]) / R
    assert _worst(f"distortion[{S}]", (got - ref).abs()[ref > 0] / (2e-6 * ref[ref > 0])) <= 1.0
    assert float(got[1]) == 0.0 and float(ref[1]) == 0.0


def _loss_inputs(R, g):
    rgb = torch.rand(R, 3, generator=g)
    image = torch.rand(R, 3, generator=g)
    vals = torch.tensor([0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0])
    sem = torch.cat([vals.repeat_interleave(2), torch.randn(R - 14, generator=g) * 3])[:R]
    mask = (torch.arange(R) % 2).float()
    return rgb, image, sem, mask


def _losses_ref(rgb, image, sem, mask):
    r = rgb.double().requires_grad_(True)
    s = sem.double().requires_grad_(True)
    mse = F.mse_loss(r, image.double())
    bce = SEM_W * F.binary_cross_entropy_with_logits(s, mask.double())
    (mse + bce).backward()
    return mse.detach(), bce.detach(), -10 * torch.log10(mse.detach()), r.grad, s.grad


def _check_loss_grads(name, R, d_rgb, d_sem, ref):
    r_rgb, r_sem = ref[3], ref[4]
    a = (d_rgb.cpu().double() - r_rgb).abs() / (1e-5 * r_rgb.abs().max(1, keepdim=True).values + 1e-300)
    b = (d_sem.cpu().double() - r_sem).abs() / (1e-5 * r_sem.abs() + SEM_W * 2.0 ** -22 / R)
    return _worst(f"{name}.d_rgb", a) <= 1.0 and _worst(f"{name}.d_sem", b) <= 1.0


@pytest.mark.parametrize("R", [1, 14, 331])
def test_losses_fwd_at_extreme_logits(dev, R):
    """k_losses: MSE, BCE (logits 0, +-1e-3, +-20, +-90 with masks 0 and 1: a BCE through log(sigmoid) overflows),
    PSNR relative 2e-6; d_rgb per ray 1e-5, d_sem per ray 1e-5 + w 2^-22 / R.  [scalars 0.056, d_rgb 0.007, d_sem 0.20]"""
    K = _K()
    g = torch.Generator().manual_seed(R)
    rgb, image, sem, mask = _loss_inputs(max(R, 14), g)
    rgb, image, sem, mask = rgb[:R].contiguous(), image[:R].contiguous(), sem[:R].contiguous(), mask[:R].contiguous()
    losses, d_rgb, d_sem = K.losses_fwd(rgb.to(dev), image.to(dev), sem.to(dev), mask.to(dev), SEM_W)
    ref = _losses_ref(rgb, image, sem, mask)
    got = losses.cpu().double()
    want = torch.stack(ref[:3])
    assert _worst(f"losses_fwd[{R}].scalars", (got - want).abs() / (2e-6 * want.abs())) <= 1.0
    assert _check_loss_grads(f"losses_fwd[{R}]", R, d_rgb, d_sem, ref)


@pytest.mark.parametrize("levels", [(256, 96), (383, 129, 447), (512, 65, 321, 1)])
@pytest.mark.parametrize("fuse", [False, True])
def test_train_losses_against_float64(dev, fuse, levels):
    """k_train_losses against float64, not only against the separate launches: the five scalars (relative 2e-6 plus the
    fixed-point term n 2^-35 — each of the n contributions is rounded to 2^-34), d_rgb / d_sem, and per proposal level
    d_wp (per ray 1e-5) or, fused, d_density (1e-4 of the two-term scale) through float64 autograd of the interlevel loss
    and get_weights, with two to four proposal levels whose E_p = ceil(S_p / 64) together cover 1 to 8.  The proposal
    densities are chosen so that get_weights gives the 2^-12-grid weights to ~1e-7, and the
    reference differentiates at those weights.  The fused d_density bound carries the upstream d_wp's own scan residue
    (E + 6) u max|d_wp| at full weight.  [scalars 0.064, d_rgb 0.009, d_sem 0.24, d_wp 0.025, d_density 0.37]"""
    K = _K()
    from fruitnerf_amd import _lib as L
    R, S_f, mult = 94, 48, 1.0
    g = torch.Generator().manual_seed(17 + fuse + 2 * len(levels))
    rgb, image, sem, mask = _loss_inputs(R, g)
    c, w = _dyadic_hist(R, S_f, g)
    prop = []
    for S_p in levels:
        cp, wp = _dyadic_hist(R, S_p, g)
        wp = wp / 2 ** math.ceil(math.log2(max(float(wp.sum(1).max()), 1e-9) + 1e-9))  # sum < 1: invertible
        ep = torch.cumsum(torch.rand(R, S_p + 1, generator=g) * 0.05 + 0.01, 1)
        delta = (ep[:, 1:] - ep[:, :-1]).double()
        T = 1 - torch.cat([torch.zeros(R, 1, dtype=F8), torch.cumsum(wp.double(), 1)[:, :-1]], 1)
        dn = (-torch.log1p(-wp.double() / T) / delta).float()
        prop.append((S_p, cp.contiguous(), wp.contiguous(), ep.contiguous(), dn.contiguous()))
    accum = torch.zeros(L.FNR_TRAIN_LOSSES_ACCUM_FLOATS, device=dev)
    lv = [(S_p, cp.to(dev), wp.to(dev)) + ((ep.to(dev), dn.to(dev)) if fuse else ()) for S_p, cp, wp, ep, dn in prop]
    losses, d_rgb, d_sem, outs = K.train_losses(rgb.to(dev), image.to(dev), sem.to(dev), mask.to(dev), SEM_W, S_f,
                                                c.to(dev), w.to(dev), lv, mult, True, accum, fuse_weights_bwd=fuse)
    ref = _losses_ref(rgb, image, sem, mask)
    il = torch.zeros((), dtype=F8)
    ref_lv = []
    for S_p, cp, wp, ep, dn in prop:
        s = dn.double().requires_grad_(True)
        w_of_s = _samples64(ep).get_weights(s[..., None])[..., 0]
        wp64 = w_of_s - w_of_s.detach() + wp.double()          # value: the grid weights; derivative: get_weights'
        wp64.retain_grad()
        loss = mult * ns.lossfun_outer(c.double(), w.double(), cp.double(), wp64).mean()
        loss.backward()
        il = il + loss.detach()
        ref_lv.append((wp64.grad, s.grad, w_of_s.detach(), ep, dn))
    dist = ns.lossfun_distortion(c.double(), w.double()).mean()
    want = torch.stack([ref[0], ref[1], ref[2], il, dist])
    n_waves = 4 * ((R + 255) // 256)
    fix = torch.tensor([n_waves * 2.0 ** -35 / (3 * R), n_waves * 2.0 ** -35 / R * SEM_W, 0.0,
                        R * len(levels) * 2.0 ** -35, R * 2.0 ** -35], dtype=F8)
    fix[2] = 10 / math.log(10) * fix[0] / want[0]
    got = losses.cpu().double()
    assert _worst(f"train_losses[fuse={fuse}].scalars", (got - want).abs() / (2e-6 * want.abs() + fix)) <= 1.0
    assert _check_loss_grads(f"train_losses[fuse={fuse}]", R, d_rgb, d_sem, ref)
    for (S_p, *_), out, (g_wp, g_s, w_s, ep, dn) in zip(prop, outs, ref_lv):
        got = out.cpu().double()
        if not fuse:
            gmax = g_wp.abs().max(1, keepdim=True).values
            assert _worst(f"train_losses.d_wp[{S_p}]", (got - g_wp).abs() / (1e-5 * gmax + 1e-30)) <= 1.0
        else:
            # the upstream d_wp is a scan of +-g terms: where it is exactly 0 in float64 the kernel's carries a residue of
            # (E + 6) u max|d_wp| of the ray, which enters the two-term scale
            E = (S_p + 63) // 64
            gw_err = (E + 6) * U * g_wp.abs().max(1, keepdim=True).values.expand_as(g_wp)
            scale, _ = _two_term_scale(ep, dn, w_s, g_wp.abs(), gw_err)
            assert _worst(f"train_losses.d_density[{S_p}]", (got - g_s).abs() / (scale + 1e-300)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# ray gradients of the sample positions
# ---------------------------------------------------------------------------------------------------------------------

AABB = torch.tensor([[-1.5, -1.0, -0.5], [1.5, 1.0, 2.5]])


def _unit_cube(p, mode):
    if mode == 0:
        return (ns.SceneContraction()(p) + 2.0) / 4.0
    return ns.get_normalized_positions(p, AABB.to(p.dtype))


def _selector(x):
    return ((x > 0.0) & (x < 1.0)).all(dim=-1)


def _ray_grad_ref(o, d, edges, g_unit, mode):
    """float64 autograd of sum g . x(p), p = Frustums.get_positions, x = contraction or AABB normalisation, times the
    selector (the producers of the unit-cube gradient apply it: zero partial where it is false)."""
    S = edges.shape[1] - 1
    o64 = o.double().requires_grad_(True)
    d64 = d.double().requires_grad_(True)
    e = edges.double()
    fr = ns.Frustums(o64[:, None, :].expand(-1, S, -1), d64[:, None, :].expand(-1, S, -1), e[:, :-1, None], e[:, 1:, None],
                     None)
    x = _unit_cube(fr.get_positions(), mode)
    sel = _selector(x)
    (x * sel[..., None] * g_unit.double()).sum().backward()
    return o64.grad, d64.grad, sel


def _ray_geometry(S, g, mode):
    """Random rays with samples out to t ~ 1000 (mode 0) or across the AABB (mode 1)."""
    R = 19
    o = torch.randn(R, 3, generator=g) * 0.5
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    if mode == 0:
        t = torch.sort(torch.rand(R, S + 1, generator=g) ** 3 * 1000.0, 1).values
        t[0] = torch.linspace(0, 0.5, S + 1)                               # a ray inside the unit ball
    else:
        t = torch.sort(torch.rand(R, S + 1, generator=g) * 4.0, 1).values
    return o.contiguous(), d.contiguous(), t.contiguous()


def _check_ray_grads(name, R, d_o, d_d, ref_o, ref_d, mag_o, mag_d):
    a = _worst(f"{name}.d_origins", (d_o.cpu().double() - ref_o).abs() / (1e-5 * mag_o + 1e-300))
    b = _worst(f"{name}.d_directions", (d_d.cpu().double() - ref_d).abs() / (1e-5 * mag_d + 1e-300))
    return a <= 1.0 and b <= 1.0


def _contrib_scale(o, d, edges, g_unit, mode):
    """Per ray: the sum over samples of |J^T g| (and times t_mid) — the magnitude of the terms the kernel adds up."""
    S = edges.shape[1] - 1
    R = o.shape[0]
    p = (o.double()[:, None, :] + d.double()[:, None, :] * (edges.double()[:, :-1, None] + edges.double()[:, 1:, None]) / 2)
    p = p.reshape(-1, 3).requires_grad_(True)
    x = _unit_cube(p, mode)
    sel = _selector(x)
    jg = torch.autograd.grad((x * sel[:, None] * g_unit.double().reshape(-1, 3)).sum(), p)[0].abs().view(R, S, 3)
    tm = ((edges.double()[:, :-1] + edges.double()[:, 1:]) / 2)[..., None]
    return jg.sum(1).max(1, keepdim=True).values, (jg * tm).sum(1).max(1, keepdim=True).values


@pytest.mark.parametrize("mode", [0, 1])
def test_position_grad_reduce_every_entry_point(dev, mode):
    """position_grad_reduce (single level and [L,N,4]), position_grad_reduce_multi (three sources, one launch) and
    position_grad_from_jacobian (Jacobian [L,3,N,2] x d_feats [L,N,2]) against float64 autograd through
    Frustums.get_positions and SceneContraction (mode 0) or get_normalized_positions (mode 1): d_origins / d_directions per
    ray within 1e-5 of the sum of the per-sample |contributions|.  [0.063]"""
    K = _K()
    warp = K.make_warp(mode, AABB.to(dev))
    g = torch.Generator().manual_seed(mode)
    sources, ok = [], True
    for S in (1, 48, 129, 512):
        o, d, t = _ray_geometry(S, g, mode)
        R = o.shape[0]
        rays = _rays(R, dev, o=o, d=d)
        partial = torch.randn(3, R * S, 4, generator=g)
        partial[..., 3] = 0.0
        x = _unit_cube((o[:, None, :] + d[:, None, :] * (t[:, :-1, None] + t[:, 1:, None]) / 2).reshape(-1, 3), mode)
        partial[:, ~_selector(x)] = 0.0
        gsum = partial.sum(0)[:, :3].view(R, S, 3)
        ref_o, ref_d, _ = _ray_grad_ref(o, d, t, gsum, mode)
        mag_o, mag_d = _contrib_scale(o, d, t, gsum, mode)
        d_o, d_d = torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
        K.position_grad_reduce(warp, rays, t.to(dev), S, partial.to(dev).contiguous(), d_o, d_d)
        ok &= _check_ray_grads(f"reduce[{mode},{S}]", R, d_o, d_d, ref_o, ref_d, mag_o, mag_d)
        # Jacobian form: g[a] = sum_l d_feats_l . J_l[a]
        Lv = 3
        jac = torch.randn(Lv, 3, R * S, 2, generator=g)
        df = torch.randn(Lv, R * S, 2, generator=g)
        gj = torch.einsum("lanf,lnf->na", jac.double(), df.double())
        gj[~_selector(x)] = 0.0
        jac[:, :, ~_selector(x)] = 0.0
        ref_o, ref_d, _ = _ray_grad_ref(o, d, t, gj.view(R, S, 3), mode)
        mag_o, mag_d = _contrib_scale(o, d, t, gj.view(R, S, 3), mode)
        d_o, d_d = torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
        K.position_grad_from_jacobian(warp, rays, t.to(dev), S, jac.to(dev).contiguous(), df.to(dev).contiguous(), d_o, d_d)
        ok &= _check_ray_grads(f"from_jacobian[{mode},{S}]", R, d_o, d_d, ref_o, ref_d, mag_o, mag_d)
        sources.append((S, o, d, t, partial, gsum))
    # multi: three sources of the same rays (same o, d), written (accumulate = 0)
    o, d = sources[0][1], sources[0][2]
    R = o.shape[0]
    srcs, ref_o, ref_d, mag_o, mag_d = [], 0, 0, 0, 0
    for S, _, _, _, _, _ in sources[1:]:
        _, _, t = _ray_geometry(S, g, mode)
        part = torch.randn(R * S, 4, generator=g)
        x = _unit_cube((o[:, None, :] + d[:, None, :] * (t[:, :-1, None] + t[:, 1:, None]) / 2).reshape(-1, 3), mode)
        part[~_selector(x)] = 0.0
        a, b, _ = _ray_grad_ref(o, d, t, part[:, :3].reshape(R, S, 3), mode)
        ma, mb = _contrib_scale(o, d, t, part[:, :3].reshape(R, S, 3), mode)
        ref_o, ref_d, mag_o, mag_d = ref_o + a, ref_d + b, mag_o + ma, mag_d + mb
        srcs.append((warp, t.to(dev).contiguous(), S, part.to(dev).contiguous()))
    d_o, d_d = torch.full((R, 3), 7.0, device=dev), torch.full((R, 3), 7.0, device=dev)
    K.position_grad_reduce_multi(srcs, _rays(R, dev, o=o, d=d), d_o, d_d, accumulate=False)
    ok &= _check_ray_grads(f"reduce_multi[{mode}]", R, d_o, d_d, ref_o, ref_d, mag_o, mag_d)
    assert ok


def _first_axis_rule(p, gu):
    """The kernel's convention in float64: at |p|_inf >= 1 the whole c'(m) (g . p) term goes to the FIRST maximal axis."""
    p, gu = p.double(), gu.double() / 4
    out = torch.empty_like(p)
    for i in range(p.shape[0]):
        a = p[i].abs()
        m = float(a.max())
        if m < 1:
            out[i] = gu[i]
            continue
        c, dc = 2 / m - 1 / m ** 2, -2 / m ** 2 + 2 / m ** 3
        j = int(torch.nonzero(a == m)[0])
        out[i] = c * gu[i]
        out[i, j] += math.copysign(1.0, float(p[i, j])) * dc * float(gu[i] @ p[i])
    return out


def test_contraction_ties_and_the_unit_norm_boundary(dev):
    """Samples where the L-inf norm of the contraction is reached by two or three coordinates (mixed signs), sit at
    |p|_inf = 1 exactly and one ulp either side of it.  One sample per ray (S = 1, origin 0,
    t0 + t1 = 2: p = d exactly in float32), so d_origins = d_directions = the per-sample gradient.

    Convention: at a tie the kernel gives the whole c'(m) (g . p) term to the FIRST maximal axis; autograd of
    torch.linalg.norm(ord=inf) splits it evenly among the tied axes.  Both are subgradients.  The kernel is not changed
    (ties occur in long runs with the camera optimiser on; another rule would change the pinned training bits), so at
    ties this asserts (1) the kernel's vector equals the float64 first-maximal-axis rule and (2) summed over the tied axes,
    sign(p_a) g_a equals autograd's value — nothing is double-counted.  Elsewhere the kernel equals autograd.  [rule 0.011]"""
    K = _K()
    one = torch.tensor(1.0)
    below, above = float(torch.nextafter(one, torch.tensor(0.0))), float(torch.nextafter(one, torch.tensor(2.0)))
    pts = torch.tensor([[1.5, -1.5, 0.2], [-3.0, 3.0, -3.0], [2.0, 0.5, -2.0], [-1.25, 0.0, 1.25], [40.0, -40.0, 40.0],
                        [1.0, 0.3, -0.5], [1.0, -1.0, 1.0], [below, 0.3, -0.2], [above, -0.3, 0.2], [0.7, below, -below],
                        [above, -above, 0.1], [0.2, 0.3, -0.9], [5.0, 1.0, -2.0], [-0.5, 700.0, 3.0]])
    R = pts.shape[0]
    g = torch.Generator().manual_seed(5)
    gu = torch.randn(R, 3, generator=g)
    gu[0] = torch.tensor([0.3, 0.7, -0.2])
    edges = torch.tensor([[0.5, 1.5]]).repeat(R, 1)
    rays = _rays(R, dev, o=torch.zeros(R, 3), d=pts)
    part = torch.cat([gu, torch.zeros(R, 1)], 1)
    d_o, d_d = torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
    K.position_grad_reduce(K.make_warp(0, AABB.to(dev)), rays, edges.to(dev), 1, part.to(dev).contiguous(), d_o, d_d)
    got = d_o.cpu().double()
    assert torch.equal(d_o.cpu(), d_d.cpu())
    ref_o, _, _ = _ray_grad_ref(torch.zeros(R, 3), pts, edges, gu[:, None, :], 0)
    rule = _first_axis_rule(pts, gu)
    a = pts.double().abs()
    m = a.max(1, keepdim=True).values
    tied = (a == m) & (m >= 1)
    n_tied = tied.sum(1)
    scale = (gu.double().abs() / 4).sum(1, keepdim=True) * (1 + m)
    assert _worst("tie.first_axis_rule", (got - rule).abs() / (1e-6 * scale)) <= 1.0
    for i in range(R):
        if n_tied[i] >= 2:
            sgn = torch.sign(pts[i].double())
            s_k = float((sgn * got[i])[tied[i]].sum())
            s_a = float((sgn * ref_o[i])[tied[i]].sum())
            assert abs(s_k - s_a) <= 1e-6 * float(scale[i]), (i, s_k, s_a)
            assert torch.allclose(got[i][~tied[i]], ref_o[i][~tied[i]], rtol=0, atol=1e-6 * float(scale[i]))
        else:
            assert torch.allclose(got[i], ref_o[i], rtol=0, atol=1e-6 * float(scale[i])), (i, got[i], ref_o[i])
    assert int((n_tied == 2).sum()) >= 3 and int((n_tied == 3).sum()) >= 2
    # the example of the issue: first-axis rule vs the even split, before the / 4
    assert torch.allclose(got[0] * 4, torch.tensor([0.456, 0.622, -0.178], dtype=F8), atol=2e-3)
    assert torch.allclose(ref_o[0] * 4, torch.tensor([0.362, 0.527, -0.178], dtype=F8), atol=2e-3)
    # AABB points on a face: the selector is false there.  It belongs to the producers of the unit-cube gradient
    # (k_hash_input_grad, the encode's Jacobian), not to this kernel, so the partial fed here is 0 as they write it:
    # this pins the float64 reference's selector on faces and that the reduction adds nothing at those samples.
    face = torch.tensor([[-1.5, 0.0, 1.0], [0.0, 1.0, 0.0], [0.3, -0.2, 2.5], [0.1, 0.2, 0.3]])
    x = ns.get_normalized_positions(face, AABB)
    sel = _selector(x)
    assert sel.tolist() == [False, False, False, True]
    gf = torch.randn(4, 3, generator=g) * sel[:, None]
    d_o, d_d = torch.zeros(4, 3, device=dev), torch.zeros(4, 3, device=dev)
    K.position_grad_reduce(K.make_warp(1, AABB.to(dev)), _rays(4, dev, o=torch.zeros(4, 3), d=face),
                           torch.tensor([[0.5, 1.5]]).repeat(4, 1).to(dev), 1,
                           torch.cat([gf, torch.zeros(4, 1)], 1).to(dev).contiguous(), d_o, d_d)
    ref_o, _, _ = _ray_grad_ref(torch.zeros(4, 3), face, torch.tensor([[0.5, 1.5]]).repeat(4, 1), gf[:, None, :], 1)
    assert torch.equal(d_o.cpu()[:3], torch.zeros(3, 3)) and torch.allclose(d_o.cpu().double(), ref_o, atol=1e-7)
