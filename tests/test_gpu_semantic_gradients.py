"""pass_semantic_gradients=True (FruitNeRF's own switch, fruit_nerf.py:56) on the GPU: the semantic loss also trains the
geometry — through the compositing weights (fruit_nerf.py:344-345, not detached) and through the geometry feature that
feeds mlp_semantics (fruit_field.py:202-203, 263-264, not detached).  Backward-only: every forward output is bit-identical
with the switch on and off.

Compositing: float64 autograd of oracle/ns_torch.py with the semantic renderer's weights attached, per element.
Field MLP backward: float64 autograd through the oracle's mlp_base_mlp -> mlp_semantics -> head on the kernel's own
features.  Model level: the CPU oracle with the switch on, at the tolerances of tests/test_gpu_training_parity.py."""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import ns_torch as ns
from tests import util
from tests.test_gpu_ray_kernels import (SEM_W, U, _composite_ref, _rays, _samples64, _two_term_scale, _weight_arith)
from tests.test_gpu_training_parity import _batch, _grad_report, _oracle_step

pytestmark = pytest.mark.gpu

# S not a multiple of 64, more than one element per lane (S > 64), ragged ray counts (R % 4 != 0)
SHAPES = [(5, 17), (33, 48), (7, 129), (33, 256)]


def _K():
    from fruitnerf_amd import _kernels as K
    return K


# ---------------------------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------------------------

def _ray_batch(R, S):
    """edges [R,S+1], density [R,S], rgb [R,S,3], logit [R,S] (float32, CPU): random rays; rows 0-3 are an empty ray, rays
    opaque at the first / last sample with composited logits +-40, and a surface spike (tests/test_gpu_ray_kernels._batch)."""
    g = torch.Generator().manual_seed(7919 * S + R)
    edges = torch.cumsum(torch.rand(R, S + 1, generator=g) * 0.05 + 0.01, 1)
    dens = torch.rand(R, S, generator=g) * (3.0 / (S * 0.035))
    rgb = torch.rand(R, S, 3, generator=g) * 1.4 - 0.2
    logit = torch.randn(R, S, generator=g) * 4.0
    dens[0] = 0.0
    dens[1, 0] = 1e8
    logit[1] = 40.0
    dens[2] = 0.0
    dens[2, -1] = 1e8
    logit[2] = -40.0
    dens[3, S // 2] = 1e7
    return edges.contiguous(), dens.contiguous(), rgb.contiguous(), logit.contiguous()


def _semgrad_ref(edges, dens, rgb, logit, g_rgb=None, g_sem=None, image=None, mask=None):
    """float64 autograd through get_weights + render_rgb_last_sample + render_semantics with the weights NOT detached.
    -> d_density, the float64 weights, gw_abs = |g_rgb| . |c_k - c_last| + |g_sem| |logit_k|, g_sem."""
    s = dens.double().requires_grad_(True)
    w = _samples64(edges).get_weights(s[..., None])
    out = ns.render_rgb_last_sample(rgb.double(), w, True)
    sem = ns.render_semantics(logit.double()[..., None], w)[:, 0]
    if image is None:
        loss = (out * g_rgb.double()).sum() + (sem * g_sem.double()).sum()
    else:
        loss = F.mse_loss(out, image.double()) + SEM_W * F.binary_cross_entropy_with_logits(sem, mask.double())
        g_rgb = 2 * (out - image.double()).detach() / out.numel()
        g_sem = SEM_W * (torch.sigmoid(sem) - mask.double()).detach() / sem.numel()
    loss.backward()
    gw_abs = (g_rgb.double().abs()[:, None, :] * (rgb.double() - rgb.double()[:, -1:, :]).abs()).sum(-1) \
        + g_sem.double().abs()[:, None] * logit.double().abs()
    return s.grad, w.detach()[..., 0], gw_abs, g_sem.double()


def _density_ratio(edges, dens, logit, sem64, w64, gw_abs, got, ref, R, inputs):
    """worst |d_density - ref| / bound: the two-term bound of tests/test_gpu_ray_kernels.py (1e-4 of the two-term scale) with
    the semantic term in gw_abs; "rounded" / "own": the launch forms g_sem from a composited logit with error sem_err (the
    classes of _check_composite_grads), an absolute error d_gs |logit_k| of the upstream gradient (gw_err)."""
    gw_err = None
    if inputs != "given":
        if inputs == "own":
            A = _weight_arith(edges, dens)
            la = logit.double().abs()
            sem_err = 2e-6 * (w64 * la).sum(1) + (A * la).sum(1)
        else:
            sem_err = U * sem64.abs()
        sig = torch.sigmoid(sem64)
        d_gs = SEM_W / R * sig * (1 - sig) * sem_err
        gw_err = d_gs[:, None] * logit.double().abs()
    scale, _ = _two_term_scale(edges, dens, w64, gw_abs, gw_err)
    return float(((got.cpu().double().view(R, -1) - ref).abs() / (scale + 1e-300)).max())


@pytest.mark.parametrize("R,S", SHAPES)
def test_composite_semgrad_backward_per_element(dev, R, S):
    """The three `_semgrad` compositing calls: d_density per element against float64 autograd with the semantic weights
    attached (two-term bound, 1e-4); d_rgb and d_logit bit-identical to the calls without the suffix; with g_sem = 0 all
    three outputs bit-identical to composite_bwd.  [measured worst err / bound: given 0.0029, targets 0.0033, fused 0.0077]"""
    K = _K()
    edges, dens, rgb, logit = _ray_batch(R, S)
    w64, c64, _, sem64 = _composite_ref(edges, dens, rgb, logit, True)
    g = torch.Generator().manual_seed(S)
    g_rgb = torch.randn(R, 3, generator=g)
    g_sem = torch.randn(R, generator=g)
    image = (c64 + 0.25).float()
    mask = (torch.arange(R) % 2).float()
    mask[1], mask[2] = 0.0, 1.0                                          # logits +-40 on the wrong side: |grad| ~ 1
    rays = _rays(R, dev)
    ev, dv, cv, lv = edges.to(dev), dens.to(dev), rgb.to(dev), logit.to(dev)
    wk = w64.float().to(dev)
    # given gradients
    parent = K.composite_bwd(rays, S, ev, dv, cv, wk, g_rgb.to(dev), g_sem.to(dev))
    got = K.composite_bwd_semgrad(rays, S, ev, dv, cv, lv, wk, g_rgb.to(dev), g_sem.to(dev))
    ref, _, gw_abs, _ = _semgrad_ref(edges, dens, rgb, logit, g_rgb, g_sem)
    worst = {"composite_bwd_semgrad": _density_ratio(edges, dens, logit, sem64, w64, gw_abs, got[0], ref, R, "given")}
    assert torch.equal(got[1], parent[1]) and torch.equal(got[2], parent[2])
    assert not torch.equal(got[0], parent[0])
    # g_sem = 0: the parent, bit for bit
    zero = torch.zeros(R, device=dev)
    for a, b in zip(K.composite_bwd_semgrad(rays, S, ev, dv, cv, lv, wk, g_rgb.to(dev), zero),
                    K.composite_bwd(rays, S, ev, dv, cv, wk, g_rgb.to(dev), zero)):
        assert torch.equal(a, b)
    # targets formed in the kernel, from the rounded float64 forward / from the launch's own forward
    ref_t, _, gw_abs_t, _ = _semgrad_ref(edges, dens, rgb, logit, image=image, mask=mask)
    c32, s32 = c64.float().to(dev), sem64.float().to(dev)
    parent = K.composite_bwd_targets(rays, S, ev, dv, cv, wk, c32, image.to(dev), s32, mask.to(dev), SEM_W)
    got = K.composite_bwd_targets_semgrad(rays, S, ev, dv, cv, lv, wk, c32, image.to(dev), s32, mask.to(dev), SEM_W)
    worst["composite_bwd_targets_semgrad"] = _density_ratio(edges, dens, logit, sem64, w64, gw_abs_t, got[0], ref_t, R,
                                                            "rounded")
    assert torch.equal(got[1], parent[1]) and torch.equal(got[2], parent[2])
    fwd_p, parent = K.composite_fwd_bwd_targets(rays, S, ev, dv, cv, lv, image.to(dev), mask.to(dev), SEM_W)
    fwd_s, got = K.composite_fwd_bwd_targets(rays, S, ev, dv, cv, lv, image.to(dev), mask.to(dev), SEM_W, semgrad=True)
    worst["composite_fwd_bwd_targets_semgrad"] = _density_ratio(edges, dens, logit, sem64, w64, gw_abs_t, got[0], ref_t, R,
                                                                "own")
    assert torch.equal(got[1], parent[1]) and torch.equal(got[2], parent[2])
    for a, b in zip(fwd_s, fwd_p):
        assert torch.equal(a, b)
    for k, v in worst.items():
        print(f"[semgrad compositing R={R} S={S}] {k}.d_density: worst |err| / bound = {v:.3g}")
    for k, v in worst.items():
        assert v <= 1.0, k


@pytest.mark.parametrize("R,S", SHAPES)
def test_composite_semgrad_launches_are_each_other(dev, R, S):
    """composite_bwd_targets_semgrad == train_losses -> composite_bwd_semgrad, and the fused forward-backward == composite_fwd
    -> composite_bwd_targets_semgrad, bit for bit (mirrors test_composite_bwd_targets_is_losses_then_composite_bwd and
    test_fused_composite_forward_backward_is_the_two_launches)."""
    from fruitnerf_amd import _lib as L
    K = _K()
    g0 = torch.Generator().manual_seed(R * 31 + S)
    o, d, pa, cam = util.random_rays(R, 7, seed=3)
    rays = K.RaysArg(o.to(dev), d.to(dev), torch.full((R, 1), 0.05, device=dev), torch.full((R, 1), 1000.0, device=dev),
                     cam.to(dev))
    euclid = torch.cumsum(torch.rand(R, S + 1, generator=g0) * 0.07 + 1e-3, dim=-1).to(dev)
    density = (torch.rand(R, S, generator=g0) ** 6 * 1e3).to(dev)
    rgb_s = torch.rand(R, S, 3, generator=g0).to(dev)
    logit_s = (torch.randn(R, S, generator=g0) * 6.0).to(dev)
    image = torch.rand(R, 3, generator=g0).to(dev)
    mask = (torch.rand(R, 1, generator=g0) > 0.5).float().to(dev)
    sem_w = 2.0
    fwd = K.composite_fwd(rays, S, euclid, density, rgb_s, logit_s, training=True)
    weights, out_rgb, acc, depth, out_sem, labels = fwd
    sp_f = torch.sort(torch.rand(R, S + 1, generator=g0), dim=-1).values.to(dev)
    accum = torch.zeros(L.FNR_TRAIN_LOSSES_ACCUM_FLOATS, device=dev)
    _, g_rgb, g_sem, _ = K.train_losses(out_rgb, image, out_sem, mask, sem_w, S, sp_f, weights.view(R, S), [], 1.0, False, accum)
    ref = K.composite_bwd_semgrad(rays, S, euclid, density, rgb_s, logit_s, weights, g_rgb, g_sem)
    got = K.composite_bwd_targets_semgrad(rays, S, euclid, density, rgb_s, logit_s, weights, out_rgb, image, out_sem, mask,
                                          sem_w)
    fwd2, got2 = K.composite_fwd_bwd_targets(rays, S, euclid, density, rgb_s, logit_s, image, mask, sem_w, semgrad=True)
    detached = K.composite_bwd_targets(rays, S, euclid, density, rgb_s, weights, out_rgb, image, out_sem, mask, sem_w)
    assert not torch.equal(got[0], detached[0])
    for name, a, b in zip(("weights", "rgb", "accumulation", "depth", "semantics", "labels"), fwd2, fwd):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} entries differ"
    for name, a, a2, b in zip(("d_density", "d_rgb", "d_logit"), got, got2, ref):
        assert float(b.abs().max()) > 0, name
        assert torch.equal(a, b), f"targets {name}: {int((a != b).sum())} of {a.numel()} entries differ"
        assert torch.equal(a2, b), f"fused {name}: {int((a2 != b).sum())} of {a2.numel()} entries differ"


# ---------------------------------------------------------------------------------------------------------------------
# field MLP backward
# ---------------------------------------------------------------------------------------------------------------------

def _field_setup(dev, shape, mode, R, S):
    K = _K()
    cfg = (util.small_config if shape == "fruit_nerf" else util.big_config)(log2=15, prop_log2=13)
    om = util.make_oracle(cfg, seed=3)
    hm = util.make_hip_like(om, dev)
    hm.field.mlp_precision = mode
    hm.train()
    hm.arena()
    fld = hm.field
    o, d, pa, cam = util.random_rays(R, 7, seed=4)
    rays = K.RaysArg(o.to(dev), d.to(dev), torch.full((R, 1), 0.05, device=dev), torch.full((R, 1), 6.0, device=dev),
                     cam.to(dev))
    _, eu = K.sample_spaced(rays, 1, S, None)
    net, gnet = fld.net_struct(), fld.net_struct(grads=True)
    feats, sel, jac = K.hash_encode_fwd(net.grid, fld.warp_struct(), rays, eu, S, want_jacobian=True)
    _, _, _, _, saved = K.field_mlp_fwd(net, rays, S, feats, sel, None, want_h=True)
    return om, hm, rays, eu, net, gnet, feats, sel, jac, saved


def _field_grads(hm):
    return {n: p.grad.detach().clone() for n, p in hm.field.named_parameters() if p.grad is not None and "hash_table" not in n}


@pytest.mark.parametrize("R,S", [(7, 40), (160, 48)])
@pytest.mark.parametrize("shape", ["fruit_nerf", "fruit_nerf_big"])
@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_field_mlp_bwd_semgrad(dev, shape, mode, R, S):
    """fnr_field_mlp_bwd_semgrad for both shapes in the three arithmetics; N = 280: tiles straddle rays, a partial 32-sample
    group of the per-wave kernels, a partial 128-sample batch of the big kernels.
    Isolation (d_density = d_rgb = 0): the parent's d_feats is exactly zero, the semgrad call's is float64 autograd of
    sum d_logit * logit through the oracle's mlp_base_mlp -> mlp_semantics -> head on the same features, at the bound
    tests/test_gpu_bf16.py::test_bf16_modes_vs_the_fp32_kernels_backward puts on this kernel's d_feats: 5e-4 of max |g|
    (bf16x3, and the fp32 chains it is compared with there), L2-relative 0.2 in plain bf16.
    [measured on an MI355X, worst err / bound over both shapes and sizes: fp32 7.2e-4, bf16x3 0.025, bf16 0.36]
    d_logit = 0: the parent bit for bit.  Everything non-zero: only the base layers and d_feats differ from the parent.
    With the Jacobian, d_position is the contraction of the returned d_feats.  Two calls: identical bits."""
    K = _K()
    om, hm, rays, eu, net, gnet, feats, sel, jac, saved = _field_setup(dev, shape, mode, R, S)
    fld = hm.field
    N = R * S
    g = torch.Generator().manual_seed(1)
    dd, dr, dl = (torch.randn(N, generator=g).to(dev), torch.randn(N, 3, generator=g).to(dev),
                  torch.randn(N, generator=g).to(dev))
    z1, z3 = torch.zeros(N, device=dev), torch.zeros(N, 3, device=dev)
    grads = hm.arena().grads

    def run(d_density, d_rgb, d_logit, semgrad, jacobian=None):
        grads.zero_()
        out = K.field_mlp_bwd(net, gnet, rays, S, feats, saved, sel, d_density, d_rgb, d_logit, jacobian=jacobian,
                              semgrad=semgrad)
        torch.cuda.synchronize()
        return out, _field_grads(hm)

    # ---- isolation
    df_p, _ = run(z1, z3, dl, False)
    assert float(df_p.abs().max()) == 0.0, "the detached form must leave d_feats untouched by the semantic loss"
    df_s, g_s = run(z1, z3, dl, True)
    assert float(df_s.abs().max()) > 0.0
    f64 = copy.deepcopy(om.field).double()
    L_, geo = feats.shape[0], f64.geo_feat_dim
    x = feats.detach().cpu().double().permute(1, 0, 2).reshape(N, 2 * L_).requires_grad_(True)
    h = f64.mlp_base_mlp(x)
    logit = f64.field_head_semantics.net(f64.mlp_semantics(h[:, 1:1 + geo]))[:, 0]
    (logit * dl.cpu().double()).sum().backward()
    ref = x.grad.view(N, L_, 2).permute(1, 0, 2)
    got = df_s.cpu().double().view_as(ref)
    if mode == "bf16":
        err, bound = float((got - ref).norm() / ref.norm()), 0.2
    else:
        err, bound = float((got - ref).abs().max() / ref.abs().max()), 5e-4
    print(f"[semgrad isolation {shape} {mode} N={N}] d_feats err {err:.3e} bound {bound:.1e} ratio {err / bound:.3g}")
    assert err <= bound
    # the base MLP's weights receive the semantic loss too
    assert all(float(g_s[n].abs().max()) > 0 for n in g_s if n.startswith("mlp_base"))

    # ---- d_logit = 0: the parent, bit for bit
    (df_p, g_p), (df_s, g_s) = run(dd, dr, z1, False), run(dd, dr, z1, True)
    assert torch.equal(df_p, df_s)
    for n in g_p:
        assert torch.equal(g_p[n], g_s[n]), n

    # ---- everything non-zero: only the base layers and d_feats differ; two calls give identical bits
    (df_p, g_p), (df_s, g_s) = run(dd, dr, dl, False), run(dd, dr, dl, True)
    df_s2, g_s2 = run(dd, dr, dl, True)
    assert not torch.equal(df_p, df_s)
    assert torch.equal(df_s, df_s2)
    for n in g_p:
        assert torch.equal(g_s[n], g_s2[n]), n
        if n.startswith("mlp_base"):
            assert not torch.equal(g_p[n], g_s[n]), n
        else:
            assert torch.equal(g_p[n], g_s[n]), n

    # ---- the input gradient rides along (test_input_gradient_inside_the_mlp_backward_is_the_separate_launch)
    (df_j, d_pos), g_j = run(dd, dr, dl, True, jacobian=jac)
    assert torch.equal(df_j, df_s)
    for n in g_s:
        assert torch.equal(g_j[n], g_s[n]), n
    a = [torch.zeros(R, 3, device=dev) for _ in range(2)]
    b = [torch.zeros(R, 3, device=dev) for _ in range(2)]
    K.position_grad_reduce(fld.warp_struct(), rays, eu, S, d_pos.view(1, N, 4), a[0], a[1])
    K.position_grad_from_jacobian(fld.warp_struct(), rays, eu, S, jac, df_j, b[0], b[1])
    torch.cuda.synchronize()
    for xg, yg in zip(a, b):
        assert float(yg.abs().max()) > 0
        err = float((xg - yg).abs().max()) / float(yg.abs().max())
        print(f"[semgrad input grad {shape} {mode} N={N}] rel err {err:.3e}")
        assert err <= 2e-6


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------

def _switch_on(cfg):
    cfg = copy.deepcopy(cfg)
    cfg.pass_semantic_gradients = True
    return cfg


@pytest.mark.parametrize("step,n_samples,shape", [(0, 48, "fruit_nerf"), (0, 40, "fruit_nerf"), (12, 48, "fruit_nerf"),
                                                  (0, 40, "fruit_nerf_big")])
def test_losses_and_all_gradients_with_semantic_gradients(dev, step, n_samples, shape):
    """tests/test_gpu_training_parity.py::test_losses_and_all_gradients with cfg.pass_semantic_gradients = True: same
    configurations, seeds, R = 160 and tolerances (2e-3 max-norm; fruit_nerf_big 2e-2 max-norm and 2e-3 L1).
    Precondition, on the oracle alone: the switch moves the gradients of mlp_base_mlp and of the hash table by more than
    100x the tolerance (of their switch-off maximum) — a switch that is not wired cannot pass."""
    from fruitnerf_amd.rays import RayBundle
    cfg = {"fruit_nerf": util.small_config, "fruit_nerf_big": util.big_config}[shape](log2=15, prop_log2=13)
    cfg.num_nerf_samples_per_ray = n_samples
    cfg.proposal_weights_anneal_max_num_iters, cfg.max_res = 1000, 2048
    tol = 2e-3 if shape == "fruit_nerf" else 2e-2
    R = 160
    o, d, pa, cam = util.random_rays(R, 7, seed=21)
    jit = [torch.rand(R, 1) for _ in range(3)]
    batch = _batch(R, 3)
    models = {}
    for on in (False, True):
        om = util.make_oracle(_switch_on(cfg) if on else cfg, seed=5)
        om.train()
        om.proposal_sampler._step = step
        om.proposal_sampler._steps_since_update = 0
        models[on] = (om,) + _oracle_step(om, o, d, pa, cam, jit, batch, step)
    om, out, ld_ref, md_ref = models[True]
    off = dict(util.named_trainable(models[False][0]))
    moved = 0
    for name, p in util.named_trainable(om):
        if name.startswith("field.mlp_base"):
            ratio = float((p.grad - off[name].grad).abs().max() / off[name].grad.abs().max())
            print(f"[semgrad oracle step={step}] {name}: switch on - off = {ratio:.3g} x max|off|")
            assert ratio > 100 * tol, name
            moved += 1
    assert moved >= 5          # two weights, two biases, the table
    for k in ld_ref:
        assert torch.equal(ld_ref[k], models[False][2][k]), k      # the switch is backward-only

    hm = util.make_hip_like(om, dev)
    assert hm.config.pass_semantic_gradients and hm.field.pass_semantic_gradients
    hm.train()
    hm.proposal_sampler._step = step
    hm.proposal_sampler._steps_since_update = 0
    hm.set_anneal(step)
    hout = hm(RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev)), jitter=[j.to(dev) for j in jit])
    hb = {k: v.to(dev) for k, v in batch.items()}
    md = hm.get_metrics_dict(hout, hb)
    ld = hm.get_loss_dict(hout, hb)
    sum(ld.values()).backward()
    torch.cuda.synchronize()
    for k in ld_ref:
        a, b = float(ld[k]), float(ld_ref[k])
        tol_l = 1e-3 * abs(b) + 1e-8 if (k == "interlevel_loss" and shape != "fruit_nerf") else 2e-5 * max(abs(b), 1e-3)
        assert abs(a - b) <= tol_l, k
    for k in md_ref:
        a, b = float(md[k]), float(md_ref[k])
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), k
    worst, worst_agg = _grad_report(om, hm, f" semgrad step={step}", with_aggregate=True)
    if shape == "fruit_nerf":
        assert worst <= 2e-3, f"worst relative gradient error {worst}"
    else:
        assert worst <= 2e-2 and worst_agg <= 2e-3, f"gradient error: max-norm {worst}, L1 {worst_agg}"


@pytest.mark.parametrize("fused", [False, True])
def test_ray_gradients_match_autograd_with_semantic_gradients(dev, fused):
    """tests/test_gpu_training_parity.py::test_ray_gradients_match_autograd with the switch on, at the same bound."""
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import fused_forward_backward
    cfg = util.small_config(log2=15, prop_log2=13)
    R = 160
    o, d, pa, cam = util.random_rays(R, 7, seed=33)
    jit = [torch.rand(R, 1) for _ in range(3)]
    batch = _batch(R, 5)
    grads = {}
    for on in (False, True):
        om = util.make_oracle(_switch_on(cfg) if on else cfg, seed=11)
        om.train()
        o_ref, d_ref = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        om.set_anneal(0)
        out = om(ns.RayBundle(o_ref, d_ref, pa.clone(), camera_indices=cam.clone()), jitter=jit)
        sum(om.get_loss_dict(out, batch).values()).backward()
        grads[on] = (o_ref.grad, d_ref.grad)
    for a, b in zip(grads[True], grads[False]):         # the switch moves the ray gradients (oracle alone)
        assert float((a - b).abs().max()) > 100 * 5e-3 * float(b.abs().max())
    hm = util.make_hip_like(om, dev)
    hm.train()
    hm.set_anneal(0)
    hb = {k: v.to(dev) for k, v in batch.items()}
    hjit = [j.to(dev) for j in jit]
    if fused:
        got = {}
        fused_forward_backward(hm, RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev)), hb, jitter=hjit, ray_grads=got)
        g_o, g_d = got["origins"], got["directions"]
    else:
        o_h, d_h = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
        hout = hm(RayBundle(o_h, d_h, pa.to(dev), cam.to(dev)), jitter=hjit)
        sum(hm.get_loss_dict(hout, hb).values()).backward()
        g_o, g_d = o_h.grad, d_h.grad
    torch.cuda.synchronize()
    for name, got_g, ref_g in (("origins", g_o, grads[True][0]), ("directions", g_d, grads[True][1])):
        scale = ref_g.abs().max().item()
        err = (got_g.cpu() - ref_g).abs().max().item()
        print(f"[semgrad ray grad fused={fused}] {name}: max|ref| {scale:.3e} max_err {err:.3e} rel {err / scale:.3e}")
        assert scale > 0 and err <= 5e-3 * scale, name


def test_forward_outputs_do_not_depend_on_the_switch(dev):
    """Train, eval, inference and export mode of FruitModel: every output tensor bit-identical with the switch on and off."""
    from fruitnerf_amd.data.fruit_datamanager import ExportDataManager
    from fruitnerf_amd.rays import RayBundle
    cfg = util.small_config(log2=14)
    R = 96
    o, d, pa, cam = util.random_rays(R, 7, seed=6)
    jit = [torch.rand(R, 1).to(dev) for _ in range(3)]
    aabb = ((-1.0, -0.6, -1.0), (1.0, 0.6, 1.0))

    def outputs(on):
        res = {}
        c = _switch_on(cfg) if on else cfg
        hm = util.make_hip_like(util.make_oracle(c, seed=2), dev)
        assert hm.config.pass_semantic_gradients is on
        rb = lambda: RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))  # noqa: E731
        hm.train()
        hm.set_anneal(0)
        res["train"] = hm(rb(), jitter=jit)
        hm.eval()
        res["eval"] = hm(rb())
        hi = util.make_hip_like(util.make_oracle(c, seed=2, test_mode="inference"), dev, test_mode="inference")
        hi.eval()
        res["inference"] = hi(rb())
        he = util.make_hip_like(util.make_oracle(c, seed=2, test_mode="export"), dev, test_mode="export")
        he.eval()
        he.setup_inference(True, 16, deterministic=True)
        dm = ExportDataManager(dev, eval_num_rays_per_batch=97)
        dm.setup_inference(aabb=aabb, num_points=16)
        res["export"] = he(dm.next_sample_volume(0)[0])
        torch.cuda.synchronize()
        return res
    off, on = outputs(False), outputs(True)
    for mode in off:
        compared = 0
        for k, v in off[mode].items():
            if torch.is_tensor(v):
                assert torch.equal(v.detach(), on[mode][k].detach()), f"{mode}: {k}"
                compared += 1
        assert compared >= 3, mode


@pytest.mark.parametrize("shape", ["fruit_nerf", "fruit_nerf_big"])
def test_fused_step_matches_the_autograd_step_with_semantic_gradients(dev, shape):
    """tests/test_gpu_training_parity.py::test_fused_step_matches_the_autograd_step with the switch on."""
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import fused_forward_backward
    cfg = _switch_on((util.small_config if shape == "fruit_nerf" else util.big_config)(log2=15, prop_log2=13))
    om = util.make_oracle(cfg, seed=9)
    R = 192
    o, d, pa, cam = util.random_rays(R, 7, seed=4)
    jit = [torch.rand(R, 1).to(dev) for _ in range(3)]
    hb = {k: v.to(dev) for k, v in _batch(R, 8).items()}
    results = []
    for fused in (False, True, None):      # None: the autograd step with the switch off
        hm = util.make_hip_like(om, dev)
        if fused is None:
            hm.config.pass_semantic_gradients = hm.field.pass_semantic_gradients = False
        hm.train()
        hm.set_anneal(0)
        rb = RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))
        if fused:
            ld, md = fused_forward_backward(hm, rb, hb, jitter=jit)
        else:
            out = hm(rb, jitter=jit)
            md = hm.get_metrics_dict(out, hb)
            ld = hm.get_loss_dict(out, hb)
            sum(ld.values()).backward()
        torch.cuda.synchronize()
        results.append((ld, md, hm.arena().grads.clone()))
    (ld_a, md_a, g_a), (ld_f, md_f, g_f), (_, _, g_off) = results
    for k in ld_a:
        assert abs(float(ld_a[k]) - float(ld_f[k])) <= 1e-6 * max(abs(float(ld_a[k])), 1e-6), k
    for k in md_a:
        assert abs(float(md_a[k]) - float(md_f[k])) <= 1e-6 * max(abs(float(md_a[k])), 1e-6), k
    scale = g_a.abs().max().item()
    assert scale > 0
    assert (g_a - g_f).abs().max().item() <= 1e-5 * scale
    assert int((g_a != 0).sum()) == int((g_f != 0).sum())
    assert (g_a - g_off).abs().max().item() > 1e-2 * scale      # the switch is wired on this path


@pytest.mark.parametrize("big", [False, True])
def test_training_steps_record_replay_and_reproduce_with_semantic_gradients(dev, big):
    """The training loop with the switch on: steps record (fnr_program_end succeeds) and the programs hold the `_semgrad`
    entry points by name; replayed training is the interpreted training bit for bit (tests/test_gpu_sequencer.py); the same
    run twice gives identical parameter bits."""
    from fruitnerf_amd import _lib as L
    from tests.test_gpu_sequencer import _interpreted, _loop

    def run(steps=40):
        loop, hm, opt, batcher, cam = _loop(dev, n_rays=1024, big=big)
        hm.config.pass_semantic_gradients = hm.field.pass_semantic_gradients = True
        losses = []
        for i in range(steps):
            ld, md = loop.step(want_metrics=(i % 3 != 0))
            losses.append(torch.stack(list(ld.values())).clone())
        torch.cuda.synchronize()
        lib = L.load()
        names = set()
        for prog in loop._programs.values():
            names |= {lib.fnr_program_op_name(prog.handle, i).decode() for i in range(lib.fnr_program_size(prog.handle))}
        return hm.arena().params.clone(), opt.exp_avg.clone(), torch.stack(losses), dict(loop.stats), names
    p1, m1, l1, stats, names = run()
    p2, m2, l2, _, _ = run()
    p_i, m_i, l_i, stats_i, _ = _interpreted(run)
    print("[semgrad sequencer] stats", stats, sorted(n for n in names if "semgrad" in n))
    assert stats["record_failed"] == 0 and stats["recorded"] >= 2 and stats["replayed"] >= 8, stats
    assert stats_i["replayed"] == 0
    assert "fnr_field_mlp_bwd_semgrad" in names
    assert "fnr_composite_bwd_targets_semgrad" in names or "fnr_composite_fwd_bwd_targets_semgrad" in names
    assert not names & {"fnr_field_mlp_bwd_adam", "fnr_composite_bwd_targets", "fnr_composite_fwd_bwd_targets"}
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(l1, l2), "two runs differ"
    assert torch.equal(p1, p_i) and torch.equal(m1, m_i) and torch.equal(l1, l_i), "replayed and interpreted steps differ"
