"""GPU: the device-side Adam / RAdam step (fnr_adam_step_spans_dev) and the torch.optim.Optimizer built on it
(engine.optimizers.ArenaAdam) — against torch.optim on the CPU, under a real torch.amp.GradScaler, in a Trainer-shaped
loop next to FusedAdam, and across checkpoints in both directions."""
import functools
import warnings

import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

# three spans of one 8192-float arena: counts 4 / 1028 / 4096, gaps between them, no start a multiple of 1024;
# (offset, count, lr, steps already taken)
N_ARENA = 8192
SPANS = [(12, 4, 1e-2, 0), (100, 1028, 3e-3, 3), (2052, 4096, 1e-3, 8)]
BOUND = {"adam": 2e-6, "radam": 5e-6}      # test_adam_matches_torch / test_radam_matches_torch: same arithmetic


def _inside():
    mask = torch.zeros(N_ARENA, dtype=torch.bool)
    for a, n, _, _ in SPANS:
        mask[a:a + n] = True
    return mask


@functools.lru_cache(maxsize=None)
def _case(n_steps=8):
    """Initial parameters and the per-step gradients (half of the entries exactly zero), shared and never modified."""
    g0 = torch.Generator().manual_seed(5)
    p0 = torch.randn(N_ARENA, generator=g0)
    grads = [torch.randn(N_ARENA, generator=g0) * (torch.rand(N_ARENA, generator=g0) > 0.5) for _ in range(n_steps)]
    return p0, grads


@functools.lru_cache(maxsize=None)
def _reference(algorithm, wd, n_steps=8):
    """torch.optim on the CPU, one instance per span with its `step` preset -> parameters after every step."""
    p0, grads = _case()
    Opt = torch.optim.Adam if algorithm == "adam" else torch.optim.RAdam
    refs, opts = [], []
    for a, n, lr, start in SPANS:
        r = p0[a:a + n].clone().requires_grad_(True)
        o = Opt([r], lr=lr, eps=1e-15, weight_decay=wd)
        o.state[r] = {"step": torch.tensor(float(start)), "exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n)}
        refs.append(r)
        opts.append(o)
    after = []
    for k in range(n_steps):
        for (a, n, _, _), r, o in zip(SPANS, refs, opts):
            r.grad = grads[k][a:a + n].clone()
            o.step()
        after.append([r.detach().clone() for r in refs])
    return after


class _Dev:
    """The arena of the kernel-level tests on the device: parameters, moments, counters, scratch."""

    def __init__(self, dev):
        p0, _ = _case()
        self.dev = dev
        self.p = p0.clone().to(dev)
        self.m, self.v = torch.zeros(N_ARENA, device=dev), torch.zeros(N_ARENA, device=dev)
        self.steps = torch.tensor([s for _, _, _, s in SPANS], dtype=torch.int64, device=dev)
        self.scalars = torch.zeros(32, device=dev)

    def step(self, grad, algorithm, wd, grad_scale=None, found_inf=None):
        from fruitnerf_amd import _kernels as K
        g = grad.to(self.dev)
        K.adam_step_spans_dev(self.p, g, self.m, self.v, [(a, n, lr) for a, n, lr, _ in SPANS], self.steps, algorithm,
                              0.9, 0.999, 1e-15, self.scalars, grad_scale=grad_scale, found_inf=found_inf, zero_grad=True,
                              weight_decay=wd)
        return g

    def snapshot(self):
        return self.p.clone(), self.m.clone(), self.v.clone(), self.steps.clone()


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("algorithm", ["adam", "radam"])
def test_device_side_step_matches_torch(dev, algorithm, wd):
    """Eight steps; the span that starts at 0 crosses RAdam's rho_t > 5 at its step 6.  A bias correction rounded to float
    on the device differs from the host-scalar kernels' by at most 1 ulp (~6e-10 lr per step): their bounds hold."""
    p0, grads = _case()
    ref = _reference(algorithm, wd)
    inside = _inside().to(dev)
    out = ~_inside()
    d = _Dev(dev)
    for k, grad in enumerate(grads):
        g = d.step(grad, algorithm, wd)
        assert float(g[inside].abs().max()) == 0.0                          # zero_grad, inside the spans ...
        assert torch.equal(g[~inside].cpu(), grad[~_inside()])              # ... and nowhere else
        assert d.steps.tolist() == [s + k + 1 for _, _, _, s in SPANS]
        worst = 0.0
        for (a, n, _, _), r in zip(SPANS, ref[k]):
            worst = max(worst, (d.p[a:a + n].cpu() - r).abs().max().item())
        print(f"[adam_step_spans_dev {algorithm} wd={wd}] step {k + 1}: max |params - torch| {worst:.3e}")
        assert worst <= BOUND[algorithm], (k, worst)
        assert torch.equal(d.p.cpu()[out], p0[out])                         # outside the spans: bit-untouched
        assert float(d.m.cpu()[out].abs().max()) == 0.0 and float(d.v.cpu()[out].abs().max()) == 0.0
    assert float(d.m.abs().max()) > 0.0


@pytest.mark.parametrize("algorithm", ["adam", "radam"])
def test_device_side_step_unscales_exactly_by_a_power_of_two(dev, algorithm):
    _, grads = _case()
    plain, scaled = _Dev(dev), _Dev(dev)
    scale = torch.full((), 65536.0, device=dev)
    for grad in grads[:3]:
        plain.step(grad, algorithm, 1e-3)
        g = scaled.step(grad * 65536.0, algorithm, 1e-3, grad_scale=scale)
        assert float(g[_inside().to(dev)].abs().max()) == 0.0
    for a, b in zip(plain.snapshot(), scaled.snapshot()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("algorithm", ["adam", "radam"])
def test_device_side_step_skips_on_found_inf(dev, algorithm):
    _, grads = _case()
    inside = _inside().to(dev)
    clean, d = _Dev(dev), _Dev(dev)
    for grad in grads[:2]:
        clean.step(grad, algorithm, 1e-3)
        d.step(grad, algorithm, 1e-3)
    before = d.snapshot()
    bad = grads[2].clone()
    bad[13], bad[150], bad[3000] = float("inf"), float("nan"), float("-inf")
    g = d.step(bad, algorithm, 1e-3, found_inf=torch.ones((), device=dev))
    for a, b in zip(before, d.snapshot()):                                  # parameters, moments, counters: untouched
        assert torch.equal(a, b)
    assert float(g[inside].abs().max()) == 0.0                              # the bad gradient does not survive
    clean.step(grads[2], algorithm, 1e-3)
    d.step(grads[2], algorithm, 1e-3, found_inf=torch.zeros((), device=dev))
    for a, b in zip(clean.snapshot(), d.snapshot()):
        assert torch.equal(a, b)


def _sync_mode_raises(dev) -> bool:
    """Does torch.cuda.set_sync_debug_mode("error") catch a host synchronisation on this build?"""
    probe = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_grad_scaler_drives_the_step_without_a_host_sync(dev):
    """A stock GradScaler (init 2^16, growth interval 2) over one arena parameter (4040 floats) and one free [10, 6]
    parameter with weight decay; an inf in iteration 3.  CPU replica: torch.optim.Adam on unscaled gradients, the bad
    iteration left out."""
    from fruitnerf_amd.engine.optimizers import ArenaAdam
    from fruitnerf_amd.params import ParamArena
    g0 = torch.Generator().manual_seed(17)
    a0, f0 = torch.randn(4040, generator=g0), torch.randn(10, 6, generator=g0)
    pa, pf = torch.nn.Parameter(a0.clone().to(dev)), torch.nn.Parameter(f0.clone().to(dev))
    arena = ParamArena([("fields", [pa])], dev)
    opt = ArenaAdam([{"params": [pa]}, {"params": [pf], "weight_decay": 1e-2}], lr=1e-2, eps=1e-15)
    ra, rf = a0.clone().requires_grad_(True), f0.clone().requires_grad_(True)
    ref = torch.optim.Adam([{"params": [ra]}, {"params": [rf], "weight_decay": 1e-2}], lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16, growth_interval=2)
    catches = _sync_mode_raises(dev)
    if not catches:
        print("[grad scaler] set_sync_debug_mode('error') does not catch .item() on this build: the no-sync assertion "
              "is not made")
    want_scale, tracker, scales = 2.0 ** 16, 0, []
    for it in range(6):
        ca, cf = torch.randn(4040, generator=g0), torch.randn(10, 6, generator=g0)
        if it == 3:
            ca[77] = float("inf")
        opt.zero_grad()
        loss = (pa * ca.to(dev)).sum() + (pf * cf.to(dev)).sum()
        scaler.scale(loss).backward()
        arena.mark_gradient("fields")             # (what the package's autograd Functions do in their backward)
        assert pa.grad.data_ptr() == arena.grads.data_ptr()
        if catches:
            torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        scaler.update()
        if it == 3:
            want_scale, tracker = want_scale / 2, 0
        else:
            tracker += 1
            if tracker == 2:
                want_scale, tracker = want_scale * 2, 0
            ra.grad, rf.grad = ca.clone(), cf.clone()
            ref.step()
        scales.append(scaler.get_scale())
        assert scales[-1] == want_scale, (it, scales)
        assert float(arena.grads.abs().max()) == 0.0 and float(pf.grad.abs().max()) == 0.0
    assert scales == [2.0 ** 16, 2.0 ** 17, 2.0 ** 17, 2.0 ** 16, 2.0 ** 16, 2.0 ** 17]
    sd = opt.state_dict()
    assert [float(sd["state"][i]["step"]) for i in (0, 1)] == [5.0, 5.0]
    assert sd["state"][0]["exp_avg"].shape == pa.shape and sd["state"][1]["exp_avg_sq"].shape == pf.shape
    ea = (pa.detach().cpu() - ra.detach()).abs().max().item()
    ef = (pf.detach().cpu() - rf.detach()).abs().max().item()
    print(f"[grad scaler] max |params - torch|: arena {ea:.3e} free {ef:.3e}")
    assert ea <= BOUND["adam"] and ef <= BOUND["adam"]


def _batch(R, seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(R, 3, generator=g), "fruit_mask": (torch.rand(R, 1, generator=g) > 0.6).float()}


def _trainer_models(dev, seed):
    cfg = util.small_config(log2=12, prop_log2=10)
    om = util.make_oracle(cfg, seed=seed)
    return om, util.make_hip_like(om, dev), util.make_hip_like(om, dev)


def test_trainer_shaped_loop_on_the_method_config_matches_fused_adam(dev):
    """Iterations 9..12, state preset as after 9 warm-up iterations (the twin of
    test_optimizer_skips_the_proposal_networks_on_steps_that_do_not_update_them): model `a` is driven the way Nerfstudio's
    Trainer drives it — Optimizers from optimizer_configs("fruit_nerf"), an enabled GradScaler — model `b` through the
    plugin loop with FusedAdam.step(skip=skipped_groups(b))."""
    from fruitnerf_amd import fruit_nerf_config as FC
    from fruitnerf_amd.engine.callbacks import TrainingCallbackAttributes, TrainingCallbackLocation as Loc
    from fruitnerf_amd.engine.optimizers import Optimizers
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import FusedAdam, skipped_groups
    om, a, b = _trainer_models(dev, 31)
    a.train()
    b.train()
    opts = Optimizers(FC.optimizer_configs("fruit_nerf"), a.get_param_groups())       # before a.arena() exists
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    hopt = FusedAdam(b)
    for m in (a, b):                              # as after 9 warm-up iterations
        m.proposal_sampler._step = 8
        m.proposal_sampler._steps_since_update = 1
    hopt.step_count = 9
    hopt.group_steps = {k: 9 for k in hopt.group_steps}
    for name, o in opts.optimizers.items():       # ... on the Trainer's side: a checkpoint of step 9 with zero moments
        sd = o.state_dict()
        sd["state"] = {i: {"step": torch.tensor(9.0), "exp_avg": torch.zeros_like(p, device="cpu"),
                           "exp_avg_sq": torch.zeros_like(p, device="cpu")}
                       for i, p in enumerate(opts.parameters[name])}
        o.load_state_dict(sd)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # (lr_scheduler.step() before optimizer.step(): the preset, not a loop)
        for s in opts.schedulers.values():
            s.last_epoch = 8
            s.step()
    cbs = {m: m.get_training_callbacks(TrainingCallbackAttributes(optimizers=None, grad_scaler=None, pipeline=None))
           for m in (a, b)}
    start = util.make_hip_like(om, dev).arena().params.clone()
    R = 96
    pa_, pb_ = a.arena().group_ranges["proposal_networks"]
    prop = opts.parameters["proposal_networks"]
    moved = []
    for step in range(9, 13):
        o, d, pa, cam = util.random_rays(R, 7, seed=300 + step)
        batch = {k: v.to(dev) for k, v in _batch(R, 70 + step).items()}
        rb = lambda: RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))  # noqa: E731
        before = a.arena().params[pa_:pb_].clone()
        state_before = None
        if step > 9:                              # (the state is placed at the first step)
            st = opts.optimizers["proposal_networks"].state
            state_before = [(st[p]["exp_avg"].clone(), st[p]["exp_avg_sq"].clone()) for p in prop]
            steps_before = [float(s["step"]) for s in opts.optimizers["proposal_networks"].state_dict()["state"].values()]
        # --- a: Trainer.train_iteration
        for cb in cbs[a]:
            cb.run_callback_at_location(step, location=Loc.BEFORE_TRAIN_ITERATION)
        opts.zero_grad_all()
        torch.manual_seed(1000 + step)            # the model draws its jitter from the device generator
        outputs = a(rb())
        loss_dict = a.get_loss_dict(outputs, batch, a.get_metrics_dict(outputs, batch))
        scaler.scale(functools.reduce(torch.add, loss_dict.values())).backward()
        opts.optimizer_scaler_step_all(scaler)
        scaler.update()
        opts.scheduler_step_all(step)
        for cb in cbs[a]:
            cb.run_callback_at_location(step, location=Loc.AFTER_TRAIN_ITERATION)
        # --- b: the plugin loop over FusedAdam
        for cb in cbs[b]:
            cb.run_callback_at_location(step, location=Loc.BEFORE_TRAIN_ITERATION)
        torch.manual_seed(1000 + step)
        outputs = b(rb())
        loss_dict = b.get_loss_dict(outputs, batch, b.get_metrics_dict(outputs, batch))
        functools.reduce(torch.add, loss_dict.values()).backward()
        hopt.step(skip=skipped_groups(b))
        for cb in cbs[b]:
            cb.run_callback_at_location(step, location=Loc.AFTER_TRAIN_ITERATION)
        torch.cuda.synchronize()
        moved.append(not torch.equal(before, a.arena().params[pa_:pb_]))
        if not moved[-1] and state_before is not None:
            st = opts.optimizers["proposal_networks"].state
            for p, (m0, v0) in zip(prop, state_before):
                assert torch.equal(st[p]["exp_avg"], m0) and torch.equal(st[p]["exp_avg_sq"], v0)
            sd = opts.optimizers["proposal_networks"].state_dict()
            assert [float(s["step"]) for s in sd["state"].values()] == steps_before
        assert float(a.arena().grads.abs().max()) == 0.0        # zeroing is fused into the step
        for p in prop:
            assert p.grad is not None                            # never detached from the gradient arena
    print("[drop-in loop] proposal networks moved on iterations 9..12:", moved)
    assert moved == [True, True, False, True]
    steps = {name: {float(s["step"]) for s in o.state_dict()["state"].values()} for name, o in opts.optimizers.items()}
    assert steps == {"proposal_networks": {12.0}, "fields": {13.0}}
    assert hopt.group_steps == {"proposal_networks": 12, "fields": 13}
    for name, o in opts.optimizers.items():
        assert o.param_groups[0]["lr"] == pytest.approx(hopt.current_lr(name), rel=4.5e-16)
        assert len(o._plan) == 1 and len(o._plan[0].spans) == 1  # a group: one span, one launch
    assert scaler.get_scale() == 65536.0
    pa_all, pb_all = a.arena().params, b.arena().params
    move = (pb_all - start).abs()
    diff = (pa_all - pb_all).abs()
    print(f"[drop-in loop] median |a - b| {diff.median().item():.3e}  mean movement {move.mean().item():.3e}")
    assert diff.median().item() <= 0.05 * move.mean().item() + 1e-7


def _small_params(dev, seed):
    g0 = torch.Generator().manual_seed(seed)
    shapes = [(64, 16), (16,), (33,), (5, 7)]
    init = [torch.randn(*s, generator=g0) for s in shapes]
    grads = [[torch.randn(*s, generator=g0) * (torch.rand(*s, generator=g0) > 0.5) for s in shapes] for _ in range(8)]
    return shapes, init, grads


def _to_cpu(sd):
    return {"state": {i: {k: v.detach().cpu().clone() for k, v in s.items()} for i, s in sd["state"].items()},
            "param_groups": sd["param_groups"]}


def test_checkpoint_goes_to_torch_optim_and_back(dev):
    from fruitnerf_amd.engine.optimizers import ArenaAdam
    from fruitnerf_amd.params import ParamArena
    shapes, init, grads = _small_params(dev, 23)

    def feed(arena, params, k):
        for p, g in zip(params, grads[k]):
            p.grad.copy_(g.to(dev))
        arena.mark_gradient("fields")

    # ArenaAdam -> torch.optim.Adam
    params = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    arena = ParamArena([("fields", params)], dev)
    opt = ArenaAdam(params, lr=1e-2, eps=1e-15, weight_decay=1e-3)
    for k in range(3):
        feed(arena, params, k)
        opt.step()
    sd = _to_cpu(opt.state_dict())
    assert [float(s["step"]) for s in sd["state"].values()] == [3.0] * len(shapes)
    assert [tuple(s["exp_avg"].shape) for s in sd["state"].values()] == shapes
    refs = [p.detach().cpu().clone().requires_grad_(True) for p in params]
    ref = torch.optim.Adam(refs, lr=1e-2, eps=1e-15, weight_decay=1e-3)
    ref.load_state_dict(sd)
    for k in range(3, 5):
        feed(arena, params, k)
        opt.step()
        for r, g in zip(refs, grads[k]):
            r.grad = g.clone()
        ref.step()
    err = max((p.detach().cpu() - r.detach()).abs().max().item() for p, r in zip(params, refs))
    print(f"[checkpoint] ArenaAdam -> torch.optim.Adam, two more steps: max |diff| {err:.3e}")
    assert err <= BOUND["adam"]

    # torch.optim.RAdam (6 steps: just past rho_t > 5) -> a fresh ArenaAdam built before the arena exists
    refs = [t.clone().requires_grad_(True) for t in init]
    ref = torch.optim.RAdam(refs, lr=1e-2, eps=1e-15)
    for k in range(6):
        for r, g in zip(refs, grads[k]):
            r.grad = g.clone()
        ref.step()
    params = [torch.nn.Parameter(r.detach().clone().to(dev)) for r in refs]
    opt = ArenaAdam(params, lr=1e-2, eps=1e-15, algorithm="radam")
    opt.load_state_dict(ref.state_dict())
    arena = ParamArena([("fields", params)], dev)               # the parameters are re-homed only now
    for k in range(6, 8):
        feed(arena, params, k)
        opt.step()
        for r, g in zip(refs, grads[k]):
            r.grad = g.clone()
        ref.step()
    assert len(opt._plan) == 1 and opt._plan[0].arena is arena and len(opt._plan[0].spans) == 1
    assert [float(s["step"]) for s in opt.state_dict()["state"].values()] == [8.0] * len(shapes)
    err = max((p.detach().cpu() - r.detach()).abs().max().item() for p, r in zip(params, refs))
    print(f"[checkpoint] torch.optim.RAdam -> ArenaAdam, two more steps: max |diff| {err:.3e}")
    assert err <= BOUND["radam"]

    # parameters of one span share its counter: their loaded steps must agree
    bad = _to_cpu(opt.state_dict())
    bad["state"][1]["step"] = torch.tensor(5.0)
    other = ArenaAdam(params, lr=1e-2, eps=1e-15, algorithm="radam")
    other.load_state_dict(bad)
    feed(arena, params, 0)
    with pytest.raises(ValueError, match="share one step counter"):
        other.step()
    arena.grads.zero_()


def test_zero_grad_keeps_arena_gradients_attached(dev):
    from fruitnerf_amd import fruit_nerf_config as FC
    from fruitnerf_amd.engine.optimizers import Optimizers
    from fruitnerf_amd.params import arena_of
    from fruitnerf_amd.rays import RayBundle
    _, hm, _unused = _trainer_models(dev, 37)
    del _unused
    hm.train()
    opts = Optimizers(FC.optimizer_configs("fruit_nerf"), hm.get_param_groups())
    arena = hm.arena()

    def attached():
        for _, p, o, n in arena.entries:
            assert arena_of(p)[0] is arena and arena_of(p)[2] == o
            assert p.grad is not None and p.grad.data_ptr() == arena.grads.data_ptr() + 4 * o

    def backward(seed):
        R = 64
        o, d, pa, cam = util.random_rays(R, 7, seed=seed)
        batch = {k: v.to(dev) for k, v in _batch(R, seed).items()}
        torch.manual_seed(seed)
        outputs = hm(RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev)))
        loss_dict = hm.get_loss_dict(outputs, batch, hm.get_metrics_dict(outputs, batch))
        functools.reduce(torch.add, loss_dict.values()).backward()

    opts.zero_grad_all()                          # (Optimizer.zero_grad(): set_to_none=True)
    attached()
    backward(1)
    assert all(float(arena.grads[a:b].abs().max()) > 0.0 for a, b in arena.group_ranges.values())
    for o in opts.optimizers.values():
        o.zero_grad(set_to_none=True)             # gradients that no step consumed: zeroed in place
    attached()
    assert float(arena.grads.abs().max()) == 0.0
    before = arena.params.clone()
    opts.optimizer_step_all()                     # nothing received a gradient since: no step
    assert torch.equal(before, arena.params)
    backward(2)
    opts.optimizer_step_all()
    attached()
    assert float(arena.grads.abs().max()) == 0.0 and not torch.equal(before, arena.params)
    backward(3)                                   # the next backward writes through the same views
    field_w = hm.field.mlp_base_mlp.layers[0].weight
    assert float(field_w.grad.abs().max()) > 0.0
    assert all(float(arena.grads[a:b].abs().max()) > 0.0 for a, b in arena.group_ranges.values())
    opts.zero_grad_all()
