"""CPU: the Nerfstudio-facing optimiser plumbing (engine.optimizers / engine.schedulers / fruit_nerf_config.
optimizer_configs) and the host-side argument checks of fnr_adam_step_spans_dev.  Nothing here needs a GPU."""
import dataclasses
import inspect

import pytest
import torch


def test_fused_optimizer_configs_have_nerfstudios_fields_and_setup():
    from fruitnerf_amd.engine import optimizers as EO
    from fruitnerf_amd import engine
    for cls, algorithm in ((EO.FusedAdamOptimizerConfig, "adam"), (EO.FusedRAdamOptimizerConfig, "radam")):
        assert [f.name for f in dataclasses.fields(cls)] == ["lr", "eps", "max_norm", "weight_decay"]
        cfg = cls(lr=3e-3, eps=1e-15)
        assert cfg.max_norm is None and cfg.weight_decay == 0
        assert list(inspect.signature(cfg.setup).parameters) == ["params"]
        p = torch.nn.Parameter(torch.zeros(8))
        opt = cls(lr=3e-3, eps=1e-15, weight_decay=1e-2).setup(params=[p])
        assert isinstance(opt, EO.ArenaAdam) and isinstance(opt, torch.optim.Optimizer) and opt.algorithm == algorithm
        g = opt.param_groups[0]
        assert g["lr"] == 3e-3 and g["eps"] == 1e-15 and g["weight_decay"] == 1e-2 and g["betas"] == (0.9, 0.999)
        # the param-group keys of this build's torch optimiser: a checkpoint written here loads there
        ref = (torch.optim.Adam if algorithm == "adam" else torch.optim.RAdam)([torch.zeros(1, requires_grad=True)])
        assert set(g) == set(ref.param_groups[0])
        assert opt._step_supports_amp_scaling and "grad_scaler" not in inspect.signature(opt.step).parameters
    assert engine.ArenaAdam is EO.ArenaAdam and engine.Optimizers is EO.Optimizers
    # param-group dicts, as torch.optim accepts them
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = EO.ArenaAdam([{"params": [a], "lr": 1e-3}, {"params": [b], "weight_decay": 1e-3}], lr=5e-4, algorithm="radam")
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 5e-4] and opt.param_groups[1]["weight_decay"] == 1e-3
    with pytest.raises(ValueError):
        EO.ArenaAdam([a], algorithm="sgd")


@pytest.mark.parametrize("method", ["fruit_nerf", "fruit_nerf_big", "fruit_nerf_huge"])
def test_optimizer_configs_carry_the_method_tables_values(method):
    from fruitnerf_amd import fruit_nerf_config as FC
    from fruitnerf_amd.engine.optimizers import FusedAdamOptimizerConfig, FusedRAdamOptimizerConfig
    table = FC.METHODS[method]["optimizers"]
    cfgs = FC.optimizer_configs(method)
    assert list(cfgs) == list(table)
    for group, o in table.items():
        c = cfgs[group]
        assert set(c) == {"optimizer", "scheduler"}
        assert type(c["optimizer"]) is (FusedAdamOptimizerConfig if o["algorithm"] == "adam" else FusedRAdamOptimizerConfig)
        assert c["optimizer"].algorithm == o["algorithm"]
        assert c["optimizer"].lr == o["lr"] and c["optimizer"].eps == o["eps"]
        assert c["optimizer"].weight_decay == o.get("weight_decay", 0) and c["optimizer"].max_norm is None
        if o.get("scheduler") is None:
            assert c["scheduler"] is None
        else:
            assert c["scheduler"].lr_final == o["scheduler"]["lr_final"]
            assert c["scheduler"].max_steps == o["scheduler"]["max_steps"]
    cam = FC.METHODS[method]["camera_optimizer"]
    c = FC.fused_optimizer_config(cam)
    assert (c.algorithm, c.lr, c.eps, c.weight_decay) == (cam["algorithm"], cam["lr"], cam["eps"], cam["weight_decay"])


def test_scheduler_stand_in_equals_exponential_decay_lr():
    """LambdaLR multiplies the initial rate by factor(step) = exponential_decay_lr(step) / lr_init: one division and one
    multiplication in double on top of the same expression, i.e. at most 2 ulp (4.5e-16 relative) apart."""
    from fruitnerf_amd.engine.schedulers import ExponentialDecaySchedulerConfig
    from fruitnerf_amd.training import exponential_decay_lr
    lr_init, lr_final, max_steps = 1e-2, 1e-4, 200000
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr_init)
    sched = ExponentialDecaySchedulerConfig(lr_final=lr_final, max_steps=max_steps).setup().get_scheduler(opt, lr_init)
    assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    for step in (0, 1, 100000, 200000, 300000):
        sched.last_epoch = step - 1
        opt.step()
        sched.step()
        want = exponential_decay_lr(step, lr_init, lr_final, max_steps)
        assert opt.param_groups[0]["lr"] == pytest.approx(want, rel=4.5e-16, abs=0.0), step
    assert opt.param_groups[0]["lr"] == pytest.approx(lr_final, rel=4.5e-16)        # constant past max_steps
    # stepped the way a Trainer does, the first iterations see lr(0), lr(1), ...
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr_init)
    sched = ExponentialDecaySchedulerConfig(lr_final=lr_final, max_steps=max_steps).get_scheduler(opt, lr_init)
    for step in range(3):
        assert opt.param_groups[0]["lr"] == pytest.approx(exponential_decay_lr(step, lr_init, lr_final, max_steps),
                                                          rel=4.5e-16)
        opt.step()
        sched.step()


def test_device_side_step_rejects_bad_arguments_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    good = (L.fnr_adam_span * 1)(L.fnr_adam_span(4, 8, 0, 1e-2, 0))

    def call(params=1, grads=1, m=1, v=1, n=1, spans=good, steps=1, algorithm=0, scalars=1):
        return lib.fnr_adam_step_spans_dev(params, grads, m, v, n, spans, steps, algorithm, 0.9, 0.999, 1e-8, None, None,
                                           0.0, 1, scalars, None)
    for kw in ({"params": None}, {"grads": None}, {"m": None}, {"v": None}, {"spans": None}, {"steps": None},
               {"scalars": None}):
        assert call(**kw) == -1 and b"adam_step_spans_dev: null" in lib.fnr_last_error(), kw
    for bad in (L.fnr_adam_span(2, 8, 0, 1e-2, 0), L.fnr_adam_span(4, 6, 0, 1e-2, 0)):     # offset / count not 4-aligned
        assert call(spans=(L.fnr_adam_span * 1)(bad)) == -1 and b"multiples of 4" in lib.fnr_last_error()
    assert call(n=0) == -1 and b"spans" in lib.fnr_last_error()
    assert call(n=L.FNR_MAX_ADAM_SPANS + 1) == -1 and b"spans" in lib.fnr_last_error()
    assert call(algorithm=2) == -1 and b"algorithm" in lib.fnr_last_error()
    assert L.FNR_ADAM_DEV_SCALAR_FLOATS == 32


def test_arena_adam_has_no_cpu_path():
    from fruitnerf_amd.engine.optimizers import ArenaAdam
    p = torch.nn.Parameter(torch.zeros(8))
    opt = ArenaAdam([p], lr=1e-2)
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(8)) and opt.state_dict()["state"] == {}
    opt.zero_grad()                                  # a parameter outside an arena: torch.optim's zero_grad
    assert p.grad is None


def test_optimizers_stand_in_builds_one_optimizer_and_scheduler_per_group():
    from fruitnerf_amd import fruit_nerf_config as FC
    from fruitnerf_amd.engine.optimizers import ArenaAdam, Optimizers
    groups = {"proposal_networks": [torch.nn.Parameter(torch.zeros(4))], "fields": [torch.nn.Parameter(torch.zeros(8))]}
    opts = Optimizers(FC.optimizer_configs("fruit_nerf_big"), groups)
    assert set(opts.optimizers) == set(groups) and set(opts.schedulers) == {"fields"}      # big: proposals unscheduled
    assert all(isinstance(o, ArenaAdam) and o.algorithm == "radam" for o in opts.optimizers.values())
    assert opts.parameters["fields"] is groups["fields"]
    sd = {k: o.state_dict() for k, o in opts.optimizers.items()}
    opts.load_optimizers(sd)                         # before any step: the state is held, not placed
    opts.zero_grad_all()
